"""Host-side half of the layer shape tests (no GPU): what tests/test_gpu_layer_shapes.py relies on is itself checked here.

  * the oracles of tests/layer_shapes.py agree with torch conv2d / interpolate / mean in float64;
  * the table reaches every path the restated launch geometry names, for 64, 256 and 304 compute units: the second pass of
    each convolution kernel's capped grid, a masked last wave, both resize kernels, stem workgroups of two and three tiles,
    the four things a sepconv run can do, every rejection; every case's buffers stay under 200 MB;
  * a correct producer passes the checks and each deliberately wrong producer (layer_shapes.MUTATIONS) is rejected on every
    case it applies to;
  * the rejections name conditions and messages that stand in the sources, in front of the launch."""
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layer_shapes as ls  # noqa: E402
from oracle import tf_ops  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deeplabv3plus-augmented-superresolution_amd", "csrc")
CUS = (64, 256, 304)
HOST_CUS = 64                                   # the data of the walk cases is built for the smallest count here


def _all(cus):
    return [c for cases in ls.table(cus).values() for c in cases]


built = lru_cache(maxsize=None)(ls.build)


@pytest.fixture(scope="module", autouse=True)
def _shared_cases():
    yield
    built.cache_clear()


# ---- the oracles ----------------------------------------------------------------------------------------------------------------
def _torch_conv(x, k, bias, stride, pad, out_hw):
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).double()
    h, w = x.shape[1:3]
    pb = max(0, (out_hw[0] - 1) * stride + 3 - pad - h)
    pr = max(0, (out_hw[1] - 1) * stride + 3 - pad - w)
    y = F.conv2d(F.pad(xt, (pad, pr, pad, pb)), torch.from_numpy(k).permute(3, 2, 0, 1).double(), torch.from_numpy(bias).double(), stride=stride)
    return y[:, :, :out_hw[0], :out_hw[1]].permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("id", ["conv-valu-w5-s2-pad0-even-relu0", "conv-valu-w6-s2-pad1-odd-relu1", "conv-mfma-w33-s1-pad1-relu0",
                                "conv-generic-w9-s1-pad1-relu1", "conv-generic-3to8-w6"])
def test_conv_oracle_agrees_with_torch_float64(id):
    c = ls.case_by_id("conv", id, HOST_CUS)
    d = built(c)
    ref = _torch_conv(d.x, d.k, d.bias, c.stride, c.pad, (c.h_out, c.w_out))
    assert np.abs(ref - d.pre64).max() <= 1e-12
    mag = _torch_conv(np.abs(d.x), np.abs(d.k), np.abs(d.bias), c.stride, c.pad, (c.h_out, c.w_out))
    assert np.allclose(d.bound, (ls.F32_GRADE if c.kernel == "mfma" else ls.GAMMA28) * mag, rtol=1e-12)


def test_stem_oracle_agrees_with_torch_float64_and_carries_layer_1s_bound():
    c = ls.case_by_id("stem", "stem-ldx4-34x50", HOST_CUS)
    d = built(c)
    mid = np.maximum(_torch_conv(d.x, d.k1, d.b1, 2, 0, (c.h_out, c.w_out)), 0)
    ref = np.maximum(_torch_conv(mid, d.k2, d.b2, 1, 1, (c.h_out, c.w_out)), 0)
    assert np.abs(ref - d.ref64).max() <= 1e-12
    e1 = ls.F32_GRADE * _torch_conv(np.abs(d.x), np.abs(d.k1), np.abs(d.b1), 2, 0, (c.h_out, c.w_out))
    zero = np.zeros(64, np.float32)
    want = ls.F32_GRADE * _torch_conv(mid, np.abs(d.k2), np.abs(d.b2), 1, 1, (c.h_out, c.w_out)) + _torch_conv(e1, np.abs(d.k2), zero, 1, 1, (c.h_out, c.w_out))
    assert np.allclose(d.bound, want, rtol=1e-10)


def test_sepconv_oracle_takes_the_fma_chain_as_its_operand():
    c = ls.case_by_id("sepconv", "sep64-act111-17x30", HOST_CUS)
    d = built(c)
    xt = torch.from_numpy(d.x).permute(0, 3, 1, 2).double().relu()
    dw = F.conv2d(xt, torch.from_numpy(d.wd).permute(2, 0, 1)[:, None].double(), torch.from_numpy(d.bd).double(), padding=1, groups=c.cin).relu()
    dw = dw.permute(0, 2, 3, 1).numpy()
    assert np.abs(d.a - dw).max() <= 10 * 2.0 ** -24 * (np.abs(dw).max() + 9 * 4 * 4)        # the float32 chain, near the float64 depthwise
    ref = np.maximum(d.a.astype(np.float64).reshape(-1, c.cin) @ d.wk.astype(np.float64) + d.bk, 0).reshape(d.ref64.shape)
    assert np.abs(ref - d.ref64).max() <= 1e-12


def test_gap_replay_is_a_mean():
    for hw, ch in ((1025, 260), (3, 252), (1, 4)):
        c = next(c for c in ls.gap_cases() if (c.h, c.cin, c.ldx) == (hw, ch, 0))
        d = built(c)
        mean = torch.from_numpy(d.x).double().mean(dim=(1, 2)).numpy().reshape(d.exact.shape)
        mag = np.abs(d.x).astype(np.float64).mean(axis=(1, 2)).reshape(d.exact.shape)
        assert (np.abs(d.exact - mean) <= (c.h // 4 + 5) * 2.0 ** -24 * mag).all()
    assert np.array_equal(ls.gap_exact(np.arange(5, dtype=np.float32).reshape(1, 5, 1)), [[np.float32(10) * (np.float32(1) / np.float32(5))]])


@pytest.mark.parametrize("id", ls.ids("resize"))
def test_resize_oracle_agrees_with_torch_and_the_float32_positions_stay_within_delta(id):
    c = ls.case_by_id("resize", id, HOST_CUS)
    d = built(c)
    ref = F.interpolate(torch.from_numpy(d.x).permute(0, 3, 1, 2).double(), size=(c.h_out, c.w_out), mode="bilinear", align_corners=False)
    assert np.abs(ref.permute(0, 2, 3, 1).numpy() - d.ref64).max() <= 1e-12
    tf = tf_ops.resize_bilinear(torch.from_numpy(d.x).double(), (c.h_out, c.w_out)).numpy()      # TF's float32 lerp weights
    assert (np.abs(tf - d.ref64) <= d.bound).all()
    assert (d.bound > 0).all()
    for n_out, n_in in ((c.h_out, c.h), (c.w_out, c.w)):
        pos, delta = ls.resize_positions(n_out, n_in)
        for p32 in ls.resize_positions_f32(n_out, n_in):
            assert (np.abs(p32.astype(np.float64) - pos) <= delta).all(), (id, n_out, n_in)


# ---- the table against the restated geometry ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cus", CUS)
def test_stem_walk_case_has_workgroups_of_two_and_three_tiles(cus):
    cases = {c.path: c for c in ls.stem_cases(cus) if c.path == "walk"}
    c = cases["walk"]
    wk = ls.stem_walk(c.b, c.h, c.w, cus)
    assert (wk.h1, wk.w1d, wk.tiles_y, wk.tiles_x) == (40, 56, 3, 4) and wk.h1 % ls.ES_T == 8 and wk.w1d % ls.ES_T == 8
    assert wk.grid == cus and 2 * cus < wk.tiles < 3 * cus
    lens = [len(t) for t in wk.of]
    assert set(lens) == {2, 3} and lens.count(3) == wk.tiles - 2 * cus
    assert all(t[1] // 12 != t[0] // 12 for t in wk.of)                        # every workgroup's tiles lie in different images
    assert sorted(t for g in wk.of for t in g) == list(range(wk.tiles))
    small = [ls.stem_walk(s.b, s.h, s.w, cus) for s in ls.stem_cases(cus) if s.path == "small"]
    assert [(s.h1, s.w1d) for s in small] == [(1, 1), (1, 20), (20, 1), (15, 15)] and all(max(len(t) for t in s.of) == 1 for s in small)


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("cin", (64, 128))
def test_sepconv_walk_cases_run_every_kind_of_run(cus, cin):
    by = {c.path: c for c in ls.sepconv_cases(cus) if c.cin == cin and c.path.startswith("walk")}
    c3, c2 = by["walk3"], by["walk2"]
    wk = ls.sepconv_walk(c3.b, c3.h, c3.w, cin, cus)
    assert (wk.tiles_y, wk.tiles_x, wk.per_image) == (2, 5, 10) and c3.h % ls.SF_TH == 4 and c3.w % ls.SF_TW == 5
    assert wk.want == cus * (2 if cin == 64 else 1) and wk.grid == wk.want and wk.per_wg == 3
    assert ls.sepconv_run_properties(wk) == dict(crosses_tile_row_end=True, crosses_image_end=True, shorter_last_run=True, idle_workgroup=True)
    assert sum(l - f for f, l in wk.runs if f < l) == wk.tiles
    wk2 = ls.sepconv_walk(c2.b, c2.h, c2.w, cin, cus)
    assert wk2.per_wg == 2 and wk2.grid == wk2.want
    p2 = ls.sepconv_run_properties(wk2)
    assert p2["crosses_tile_row_end"] and p2["idle_workgroup"]                 # (pairs of tiles never straddle an image of ten)
    for c in ls.sepconv_cases(cus):
        if c.cin == cin and not c.path.startswith("walk"):
            assert ls.sepconv_walk(c.b, c.h, c.w, cin, cus).per_wg == 1
    assert {c.act for c in ls.sepconv_cases(cus) if c.cin == cin} == set(ls.ACTS)
    assert {(c.h, c.w) for c in ls.sepconv_cases(cus) if c.cin == cin and c.path == "small"} == set(ls.SMALL_MAPS)


def test_conv_cases_reach_the_second_pass_the_masked_wave_and_every_ragged_width():
    cases = ls.conv_cases()
    for kernel in ("valu", "mfma", "generic"):
        mine = [c for c in cases if c.kernel == kernel]
        assert all(ls.conv_kernel(ls.entry_of(c), c.cin, c.cout) == kernel for c in mine)
        (sp,) = [c for c in mine if c.path == "second_pass"]
        wk = ls.conv_work(kernel, sp.b, sp.h_out, sp.w_out, sp.cout)
        assert wk.grid == ls.CAP_BLOCKS and wk.passes == 2 and wk.first_pass_groups < wk.groups and sp.b > 1
        if kernel == "valu":
            assert wk.groups % 8 and wk.masked_groups == 3
        assert all(ls.conv_work(kernel, c.b, c.h_out, c.w_out, c.cout).passes == 1 for c in mine if c is not sp)
        assert {(c.stride, c.pad, c.h % 2) for c in mine} >= {(2, 0, 0), (2, 1, 1), (1, 1, 1)}
        assert {c.relu for c in mine} == {0, 1, 2}
        assert any(c.ldx == 4 for c in mine) and any(c.ldy == 48 and c.lead == 16 for c in mine)
    assert {c.w_out % 4 for c in cases if c.kernel == "valu" and c.path == "ragged"} == {1, 2, 3}
    assert {c.w_out for c in cases if c.kernel == "valu" and c.w_out < ls.SP} == {1, 2, 3}
    assert {c.w_out for c in cases if c.kernel == "mfma" and c.path == "ragged"} == {1, 31, 33, 70}
    assert {(c.cin, c.cout) for c in cases if c.kernel == "generic"} == {(2, 4), (3, 8)}
    assert ls.cap_grid(0) == 1 and ls.cap_grid(257) == 2 and ls.cap_grid(10 ** 9) == 8192
    for c in cases:                                                       # asr_conv3x3_stem_f16x3 accepts them: the output fits the input
        assert (c.h_out - 1) * c.stride - c.pad + 2 < c.h + 2 and (c.w_out - 1) * c.stride - c.pad + 2 < c.w + 2


def test_relu6_cases_reach_both_pieces_of_the_clamp():
    cases = [c for c in ls.conv_cases() if c.relu == 2 and c.path != "second_pass"]
    assert {c.kernel for c in cases} == {"valu", "mfma", "generic"}
    for c in cases:
        below, above = ls.relu6_reach(built(c))
        assert below >= 1 and above >= 1, (c.id, below, above)


def test_gap_and_resize_cases_cover_the_issue():
    gap = ls.gap_cases()
    assert {c.h for c in gap} == {1, 3, 5, 1025} and {c.cin for c in gap} == {4, 252, 260, 320} and {c.b for c in gap} == {1, 3}
    assert {(c.h, c.cin) for c in gap if not c.ldx} == {(hw, ch) for hw in (1, 3, 5, 1025) for ch in (4, 252, 260, 320)}
    assert any(c.ldx == c.cin + 12 for c in gap) and {-(-c.cin // 256) for c in gap} == {1, 2}
    rs = ls.resize_cases()
    x4 = [c for c in rs if c.kernel == "x4"]
    assert all(ls.resize_kernel(c.w, c.w_out) == c.kernel == c.path for c in rs)
    assert {c.w for c in x4} == {2, 3, 9} and all((c.w * c.cin // 4) % 256 for c in x4)
    assert {c.h_out / c.h for c in x4 if c.h == 4} == {4, 2, 1, 2.5, 0.5} and any(c.h == 1 for c in x4)
    assert any(c.ldx > c.cin and c.ldy > c.cin for c in x4) and any(c.w * c.cin // 4 > 256 for c in x4)
    gen = {c.id: c for c in rs if c.kernel == "generic"}
    assert (gen["resize-gen-w1to4"].w, gen["resize-gen-w1to4"].w_out) == (1, 4)
    assert any((c.h, c.w, c.h_out, c.w_out) == (1, 1, 5, 7) for c in gen.values()) and any(c.h_out < c.h and c.w_out < c.w for c in gen.values())
    assert any(c.w_out == 3 * c.w for c in gen.values()) and any(c.w_out == 2.5 * c.w for c in gen.values()) and any(c.cin == 4 for c in gen.values())


@pytest.mark.parametrize("cus", CUS)
def test_ids_do_not_depend_on_the_cu_count_and_buffers_stay_small(cus):
    for family in ls.FAMILIES:
        assert [c.id for c in ls.FAMILIES[family](cus)] == ls.ids(family)
    cases = _all(cus)
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        assert c.bytes < 200e6, (c.id, c.bytes)
        assert c.lead % 4 == 0 and c.ld_out % 4 == 0                       # the output pointer stays 16-byte aligned


# ---- the checks and the mutants ------------------------------------------------------------------------------------------------------
HOST_CASES = _all(HOST_CUS)


@pytest.mark.parametrize("case", HOST_CASES, ids=[c.id for c in HOST_CASES])
def test_a_correct_producer_passes_every_check(case):
    d = built(case)
    ratio = ls.check_buffer(d, ls.produce(d, cus=HOST_CUS))
    assert ratio <= 0.5                                                     # one float32 rounding of the reference: far inside every bound


@pytest.mark.parametrize("mutation", ls.MUTATIONS)
def test_every_wrong_producer_is_rejected(mutation):
    cases = [c for c in HOST_CASES if ls.applies(c, mutation)]
    need = {"stem_second_tile_from_first_tiles_intermediate": 1, "sepconv_halo_row_from_previous_prefetch": 4, "second_pass_unwritten": 3,
            "relu6_as_relu": 3, "write_into_gap_channels": 7}.get(mutation, 50)
    assert len(cases) >= need, (mutation, len(cases))
    for c in cases:
        d = built(c)
        buf = ls.produce(d, mutation, cus=HOST_CUS)
        with pytest.raises(AssertionError):
            ls.check_buffer(d, buf)
            pytest.fail(f"{mutation} passed every check on {c.id}", pytrace=False)


# ---- the rejections against the sources ------------------------------------------------------------------------------------------------
def _entry_body(entry):
    for name in ("layers.hip", "sepconv.hip"):
        text = open(os.path.join(CSRC, name)).read()
        m = re.search(r'extern "C" int ' + entry + r"\(", text)
        if m:
            nxt = text.find('extern "C"', m.end())
            return text[m.start():nxt if nxt > 0 else len(text)]
    raise AssertionError(entry)


@pytest.mark.parametrize("r", ls.REJECTS, ids=[r.id for r in ls.REJECTS])
def test_every_rejection_stands_in_the_source_in_front_of_the_launch(r):
    assert ls.reject_condition_holds(r)
    body = _entry_body(r.entry)
    at = body.find(r.message.replace("%", "%%"))
    assert at > 0, r.message
    macro_at = max(body.rfind("ASR_UNSUPPORTED(", 0, at), body.rfind("ASR_REQUIRE(", 0, at))
    assert body[macro_at:].startswith(r.macro + "(")
    assert r.rc == (ls.ASR_ERR_UNSUPPORTED if r.macro == "ASR_UNSUPPORTED" else ls.ASR_ERR_INVALID_ARG)
    launch = min(i for i in (body.find("hipLaunchKernelGGL"), body.find("launch_sepconv_fused<")) if i >= 0)
    assert at < launch
    assert len(r.ints) + r.nptr + 1 == body[:body.find(")")].count(",") + 1       # the argument count of the entry point


def test_the_rejections_cover_the_issue():
    ids = {r.id for r in ls.REJECTS}
    assert ids >= {"stem-odd-h", "stem-odd-w", "stem-misaligned-w2", "sep-cin96", "sep-cout64", "sep-ldx66", "sep-misaligned-x",
                   "mfma-stem-output-does-not-fit", "direct-weights-beyond-lds", "direct-cout6", "gap-c6"}


def test_the_restated_constants_stand_in_the_sources():
    layers = open(os.path.join(CSRC, "layers.hip")).read()
    sep = open(os.path.join(CSRC, "sepconv.hip")).read()
    assert f"constexpr int ES_T = {ls.ES_T}," in layers and f"constexpr int SP = {ls.SP};" in layers
    assert "return (int)(g < 8192 ? (g > 0 ? g : 1) : 8192);" in layers and "asr_cdiv(total, 256)" in layers
    assert "const int grid = (int)(tiles < cus ? tiles : cus);" in layers and "tile += gridDim.x" in layers
    assert "if (w_out == 4 * w_in && w_in >= 2) {" in layers and "if (cin == 3 && cout == 32) {" in layers
    assert f"constexpr int SF_TH = {ls.SF_TH}, SF_TW = {ls.SF_TW}," in sep
    assert "const long long want = (long long)cus * (lds <= 80 * 1024 ? 2 : 1);" in sep and "// 128 KB (cin 128) / 64 KB (cin 64)" in sep
    assert "const long long per_wg = (total + gridDim.x - 1) / gridDim.x;" in sep
    assert "first = (long long)blockIdx.x * per_wg, last = min(first + per_wg, total);" in sep
