"""asr_realign_covered_f32 (csrc/sr.hip: sr_realign_covered_kernel, sr_realign_covered_median_kernel): the sum of the realigned
values over the sum of the realigned weights, the median over the copies that saw a pixel, and the coverage map, held bit for
bit to the rule of include/asr_hip.h.

The yardstick is the library's own per-copy value: one asr_realign_max_f32 call on a stack viewed as [B * n, 1, h, w] folds ONE
copy per output plane, so it returns the n warped planes themselves.  Applied once to y and once to wgt it gives v_i and c_i,
and the rule is restated on them in numpy float32: sequential sums, one division, a sort of the valid values."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from oracle import tf_ops

pytestmark = pytest.mark.gpu

SHAPES = (((64, 64), (16, 16)), ((48, 80), (12, 20)), ((50, 70), (16, 16)),      # f = 4 square and rectangle, a non-multiple
          ((3, 33), (2, 9)), ((3, 65), (2, 17)))                                    # one live lane / row in the last tiles
SMALL_SHAPES = (((8, 8), (4, 4)), ((3, 33), (2, 9)), ((3, 65), (2, 17)))            # for n at the cap
CASES = ("wide", "trans", "proj")
KINDS = ("uniform", "mask")
WGTS = ("ones", "random", "validity")
SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(("mean", "median", "cov"), r)]
OUT_OF_FRAME = 3                          # the copy shifted by (1.5 W, -1.5 H) when n > 3
F32 = np.float32


def _proj_range(tf8, H, W):
    c = np.asarray(tf8, np.float64).reshape(-1, 8)
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    p = c[:, 6:7] * corners[:, 0] + c[:, 7:8] * corners[:, 1] + 1.0
    return float(p.min()), float(p.max())


def _transforms(case, batch, n, H, W, seed):
    """(trans_tf, rot_tf [batch, n, 8], angles [batch, n], shifts [batch, n, 2]) of translate(-shifts) / rotate(-angles) as the
    reference builds them: angles U(-0.6, 0.6) rad, shifts U(-0.4, 0.4) of the frame; copy 0 the identity, copy 1 an integer
    shift, copy 3 wholly out of frame.  "trans": an affine-but-not-pure translate stage on copy 2 and projective terms in copy
    4's; "proj": projective terms in the rotations of copies 1 and 2."""
    rng = np.random.default_rng(seed)
    trs, rots, angs, shs = [], [], [], []
    for _ in range(batch):
        ang = rng.uniform(-0.6, 0.6, n).astype(F32)
        sh = (rng.uniform(-0.4, 0.4, (n, 2)) * [W, H]).astype(F32)
        ang[0] = 0
        sh[0] = 0
        if n > 1:
            sh[1] = np.round(sh[1])
        if n > OUT_OF_FRAME:
            sh[OUT_OF_FRAME] = [1.5 * W, -1.5 * H]
        tr = tf_ops.translations_to_projective_transforms(-sh)
        rot = tf_ops.angles_to_projective_transforms(-ang, H, W)
        if case == "trans":
            if n > 2:
                tr[2, :2] = [1.05, 0.03]
            if n > 4:
                tr[4, 6:] = [0.9e-3, -1.2e-3]
        elif case == "proj":
            if n > 1:
                rot[1, 6:] = [-1.1e-3, 0.8e-3]
            if n > 2:
                rot[2, 6:] = [0.6e-3, 1.4e-3]
        else:
            assert case == "wide"
        for t in (tr, rot):
            lo, hi = _proj_range(t, H, W)
            assert 0.5 <= lo and hi <= 1.5
        trs.append(tr), rots.append(rot), angs.append(ang), shs.append(sh)
    return np.stack(trs).astype(F32), np.stack(rots).astype(F32), np.stack(angs), np.stack(shs)


def _inputs(kind, batch, n, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":                 # smooth enough, signed
        return rng.uniform(-2.0, 2.0, (batch, n, h, w)).astype(F32)
    # {0, 1} masks of one object whose edges move by a pixel from copy to copy: plateaus of ties at 0 and at 1
    y = np.zeros((batch, n, h, w), F32)
    for b in range(batch):
        for i in range(n):
            t, l = h // 4 + rng.integers(-1, 2), w // 4 + rng.integers(-1, 2)
            y[b, i, t:t + h // 2 + rng.integers(0, 2), l:l + w // 2 + rng.integers(0, 2)] = 1.0
    return y


def _planes(xd, trd, rotd, hw):
    """[B, n, H, W]: asr_realign_max_f32 over single-copy "stacks" -- the per-copy planes of the parent commit's kernel."""
    from asr_amd import ops
    b, n, h, w = xd.shape
    s = ops.realign(xd.contiguous().view(b * n, 1, h, w), trd.view(b * n, 1, 8), rotd.view(b * n, 1, 8), hw, "max")
    return s.view(b, n, hw[0], hw[1]).cpu().numpy()


def _rule(V, Cw, cov_min=0.5, valid_min=0.5):
    """The header's rule on the per-copy planes V, Cw [B, n, H, W] in float32 -> dict(mean, median, cov)."""
    assert V.dtype == F32 and Cw.dtype == F32
    n = V.shape[1]
    S, C = np.zeros_like(V[:, 0]), np.zeros_like(V[:, 0])
    for i in range(n):                                    # copy order
        S = S + V[:, i]
        C = C + Cw[:, i]
    assert S.dtype == F32 and C.dtype == F32
    ok = C >= F32(cov_min)
    mean = np.where(ok, S / np.where(ok, C, F32(1)), F32(0)).astype(F32)      # one IEEE division
    valid = Cw >= F32(valid_min)
    nv = valid.sum(axis=1)
    s = np.sort(np.where(valid, V, F32(np.inf)), axis=1)                      # the valid values first, sorted
    lo, hi = np.maximum(nv - 1, 0) // 2, nv // 2
    a = np.take_along_axis(s, lo[:, None], axis=1)[:, 0]
    c = np.take_along_axis(s, np.minimum(hi, n - 1)[:, None], axis=1)[:, 0]
    with np.errstate(invalid="ignore"):
        mid = a + (c - a) * F32(0.5)                                           # two roundings
    median = np.where(nv > 0, np.where(lo == hi, a, mid), F32(0)).astype(F32)
    return {"mean": mean, "median": median, "cov": C}


class _Problem:
    def __init__(self, shape, case, kind, wgt, n, batch, seed=170):
        from asr_amd import ops
        from asr_amd.superresolution_scripts.augmentation_utils import copy_validity
        (H, W), (h, w) = shape
        self.H, self.W, self.h, self.w, self.n, self.batch = H, W, h, w, n, batch
        self.tag = f"{H}x{W}<-{h}x{w}/{case}/{kind}/{wgt}/n={n}/B={batch}"
        self.y = _inputs(kind, batch, n, h, w, seed)
        self.tr, self.rot, self.ang, self.sh = _transforms(case, batch, n, H, W, seed + 1)
        self.yd, self.trd, self.rotd = ops.to_device(self.y), ops.to_device(self.tr), ops.to_device(self.rot)
        if wgt == "ones":
            self.wd = torch.ones((h, w), dtype=torch.float32, device=self.yd.device)
            full = self.wd.expand(batch, n, h, w)
        elif wgt == "random":
            self.wd = ops.to_device(np.random.default_rng(seed + 2).uniform(0.0, 1.0, (batch, n, h, w)).astype(F32))
            full = self.wd
        else:
            self.wd = torch.stack([copy_validity(self.ang[b], self.sh[b], (H, W), (h, w)) for b in range(batch)]).contiguous()
            assert tuple(self.wd.shape) == (batch, n, h, w) and float(self.wd.min()) >= 0.0 and float(self.wd.max()) <= 1.0
            full = self.wd
        self.V = _planes(self.yd, self.trd, self.rotd, (H, W))
        self.C = _planes(full, self.trd, self.rotd, (H, W))
        for a in (self.V, self.C):
            assert np.isfinite(a).all()
            a.setflags(write=False)
        if n > OUT_OF_FRAME:
            assert not self.V[:, OUT_OF_FRAME].any() and not self.C[:, OUT_OF_FRAME].any()

    def covered(self, want=("mean", "median", "cov"), wd=None, **kw):
        from asr_amd import ops
        out = ops.realign_covered(self.yd, self.wd if wd is None else wd, self.trd, self.rotd, (self.H, self.W), want=want, **kw)
        assert set(out) == set(want)
        return {k: v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _cap():
    from asr_amd import _lib
    return _lib.load().asr_realign_select_max_copies()


N_ALL = [1, 2, 5, 64, 65, 100, "cap"]


def _problems(n_index):
    """Every (shape, weight kind) pair for this n; the transform case, the input kind and the batch (1 or 3) rotate with the
    pair and with n, so that over the seven n each of them meets every shape and every weight kind."""
    n = N_ALL[n_index]
    shapes = SHAPES
    if n == "cap":
        n, shapes = _cap(), SMALL_SHAPES
    for idx, (shape, wgt) in enumerate(itertools.product(shapes, WGTS)):
        yield _Problem(shape, CASES[(idx + n_index) % 3], KINDS[(idx // 3 + n_index) % 2], wgt, n, (1, 3)[(idx + n_index) % 2])


@pytest.mark.parametrize("n_index", range(len(N_ALL)), ids=[str(n) for n in N_ALL])
def test_the_rule_bit_for_bit(dev, n_index):
    """out_mean, out_cov and out_median equal the numpy rule on the per-copy planes exactly, at the default thresholds and at
    (cov_min, valid_min) = (2, 0.25); every requested subset of the three outputs carries the bits of the full call."""
    invalid_seen = low_cov_seen = ties = 0
    for p in _problems(n_index):
        for kw in (dict(), dict(cov_min=2.0, valid_min=0.25)):
            want = _rule(p.V, p.C, **kw)
            got = p.covered(**kw)
            for k in ("cov", "mean", "median"):
                assert got[k].shape == (p.batch, p.H, p.W) and got[k].dtype == F32
                assert np.array_equal(got[k], want[k]), (p.tag, kw, k, int((got[k] != want[k]).sum()))
            low_cov_seen += int((want["cov"] < F32(kw.get("cov_min", 0.5))).sum())
        invalid_seen += int((p.C < F32(0.5)).sum())
        if "/mask/" in p.tag:
            ties += int((_rule(p.V, p.C)["median"] == 1.0).sum())
        full = p.covered()
        for sub in SUBSETS:
            part = p.covered(want=sub)
            for k in sub:
                assert np.array_equal(part[k], full[k]), (p.tag, sub, k)
    assert invalid_seen > 0               # copies that did not see a pixel do occur
    if N_ALL[n_index] != "cap":
        assert ties > 0                   # and so do medians on a plateau of ties (not asked of the tiny planes at the cap)
    if N_ALL[n_index] == 5:
        assert low_cov_seen > 0           # with five copies, one of them out of frame, some pixels stay below cov_min


@pytest.mark.parametrize("n,batch", [(5, 3), (100, 1)])
def test_shared_plane(dev, n, batch):
    """wgt_shared = 1 with plane P equals wgt_shared = 0 with P broadcast to [B, n, h, w], bit for bit."""
    from asr_amd import ops
    for shape in SHAPES[1:4]:
        p = _Problem(shape, "wide", "uniform", "ones", n, batch)
        plane = ops.to_device(np.random.default_rng(9).uniform(0.0, 1.0, (p.h, p.w)).astype(F32))
        shared = p.covered(wd=plane)
        spread = p.covered(wd=plane.expand(batch, n, p.h, p.w).contiguous())
        for k in shared:
            assert np.array_equal(shared[k], spread[k]), (p.tag, k)
        assert (shared["cov"] > 0).any() and (shared["median"] != 0).any()


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 100])
def test_ends(dev, n):
    """Identity transforms, H = 4h, a shared ones plane: every copy sees every pixel, so out_cov is exactly n, out_mean is
    asr_realign_mean_f32 and out_median is asr_realign_select_f32 at the median's ranks, bit for bit, odd and even n."""
    from asr_amd import ops
    for (h, w), kind, batch in (((16, 16), "uniform", 1), ((12, 20), "mask", 3)):
        H, W = 4 * h, 4 * w
        yd = ops.to_device(_inputs(kind, batch, n, h, w, 31))
        tr = ops.to_device(np.broadcast_to(tf_ops.translations_to_projective_transforms(np.zeros((n, 2), F32)), (batch, n, 8)).astype(F32))
        rot = ops.to_device(np.broadcast_to(tf_ops.angles_to_projective_transforms(np.zeros(n, F32), H, W), (batch, n, 8)).astype(F32))
        ones = torch.ones((h, w), dtype=torch.float32, device=yd.device)
        out = ops.realign_covered(yd, ones, tr, rot, (H, W), want=("mean", "median", "cov"))
        assert torch.equal(out["cov"], torch.full_like(out["cov"], float(n)))
        assert torch.equal(out["mean"], ops.realign(yd, tr, rot, (H, W), "mean"))
        q, _ = ops.realign_select(yd, tr, rot, (H, W), ranks=[ops.quantile_ranks(n, 0.5)])
        assert np.array_equal(out["median"].cpu().numpy(), q[0].cpu().numpy())


def _test_sr_draws(n=100, size=128, angle_max=0.15, shift_max=20, seed=1234):
    from asr_amd.superresolution_scripts.augmentation_utils import draw_augmentation_parameters
    np.random.seed(seed)
    return draw_augmentation_parameters(n, angle_max, shift_max)


def _sr(feature_size, output_size, n, **kw):
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    return Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=3, num_aug=n, optimizer=opt, feature_size=feature_size,
                           output_size=output_size, **kw)


def test_constant_in_constant_out(dev):
    """y = 1 and wgt = 1 (shared) under scripts/test_SR.py's draws scaled to 128 <- 32 (N = 100, shifts up to 20 px, angles up to
    0.15 rad): S and C are the same sums, so out_mean is exactly 1 wherever out_cov >= cov_min and exactly 0 elsewhere, while
    the plain mean of the same input falls below 0.5.  A copy that saw a pixel whole has c_i = v_i = 1 exactly (the two tap
    weights of a bilinear sample are exact and add up to 1), so at valid_min = 1 out_median is exactly 1 wherever a valid copy
    exists.  At the default valid_min = 0.5 a copy whose seam crosses the pixel is valid with 0.5 <= v_i < 1: the median is 1
    where the copies that saw the pixel whole are the majority of the valid ones, and within [0.5, 1] elsewhere (the rule's
    answer at the few pixels that only seams reach)."""
    from asr_amd import ops
    n, S, s = 100, 128, 32
    angles, shifts = _test_sr_draws()
    sr = _sr((s, s), (S, S), n)
    rot, tr = sr._transforms(angles[None], shifts[None], dev, negate=True)
    yd = torch.ones((1, n, s, s), dtype=torch.float32, device=dev)
    ones = torch.ones((s, s), dtype=torch.float32, device=dev)
    plain = ops.realign(yd, tr, rot, (S, S), "mean").cpu().numpy()
    assert plain.min() < 0.5
    c_i = _planes(yd, tr, rot, (S, S))[0]                                   # [n, S, S]
    for cov_min in (0.5, 10.0, 60.0):
        out = {k: v.cpu().numpy() for k, v in
               ops.realign_covered(yd, ones, tr, rot, (S, S), want=("mean", "cov"), cov_min=cov_min).items()}
        seen = out["cov"] >= F32(cov_min)
        assert np.array_equal(out["mean"], np.where(seen, F32(1), F32(0))), cov_min
        assert seen.any()
    assert not seen.all()                                                    # cov_min = 60: the corners are below it
    med1 = ops.realign_covered(yd, ones, tr, rot, (S, S), want=("median",), valid_min=1.0)["median"].cpu().numpy()[0]
    any_whole = (c_i >= F32(1)).any(axis=0)
    assert any_whole.any() and np.array_equal(med1, np.where(any_whole, F32(1), F32(0)))
    med = ops.realign_covered(yd, ones, tr, rot, (S, S), want=("median",))["median"].cpu().numpy()[0]
    valid = c_i >= F32(0.5)
    nv, whole = valid.sum(axis=0), (c_i == F32(1)).sum(axis=0)
    assert (med[2 * whole > nv + 1] == 1.0).all() and (2 * whole > nv + 1).mean() > 0.9
    assert ((med[nv > 0] >= 0.5) & (med[nv > 0] <= 1.0)).all() and (med[nv == 0] == 0).all()


def test_nobody_saw_it(dev):
    """Every copy shifted out of frame by +-W: all three outputs are 0 everywhere.  With one copy left in place, mean and
    median are that copy's plane where it is in frame."""
    from asr_amd import ops
    n, (H, W), (h, w) = 6, (48, 80), (12, 20)
    y = _inputs("uniform", 2, n, h, w, 5)
    sh = np.zeros((2, n, 2), F32)
    sh[..., 0] = np.where(np.arange(n) % 2 == 0, W, -W)[None]
    sh[0, :, 1] = np.where(np.arange(n) % 3 == 0, H, 0)
    ang = np.zeros((2, n), F32)
    ones = torch.ones((h, w), dtype=torch.float32, device=dev)
    rnd = ops.to_device(np.random.default_rng(6).uniform(0.5, 1.0, (2, n, h, w)).astype(F32))

    def run(sh, wd):
        tr = ops.to_device(np.stack([tf_ops.translations_to_projective_transforms(-sh[b]) for b in range(2)]).astype(F32))
        rot = ops.to_device(np.stack([tf_ops.angles_to_projective_transforms(-ang[b], H, W) for b in range(2)]).astype(F32))
        yd = ops.to_device(y)
        out = ops.realign_covered(yd, wd, tr, rot, (H, W), want=("mean", "median", "cov"))
        return {k: v.cpu().numpy() for k, v in out.items()}, _planes(yd, tr, rot, (H, W))

    for wd in (ones, rnd):
        out, _ = run(sh, wd)
        for k, v in out.items():
            assert not v.any(), k
    sh2 = sh.copy()
    sh2[:, 4] = [7.0, -3.0]                                  # copy 4 stays (partly) in frame
    out, V = run(sh2, ones)
    in_frame = out["cov"] >= F32(0.5)
    assert in_frame.any() and not in_frame.all()
    assert np.array_equal(out["median"][in_frame], V[:, 4][in_frame])
    whole = out["cov"] == F32(1)
    assert whole.any() and np.array_equal(out["mean"][whole], V[:, 4][whole])
    assert not out["mean"][~in_frame].any() and not out["median"][~in_frame].any()


def test_what_it_is_for(dev):
    """A perfect network on an object in the image corner (y > 90 & x > 80 on 128 x 128): N = 100 copies under
    np.random.seed(1234), shifts up to 20 px, angles up to 0.15 rad, resized to 32 x 32 and binarised at 0.5; IoU of
    x > 0.5 * max(x) against the object.  The CPU oracle (oracle/augment.py + oracle/sr.py, the rule in numpy) gives for these
    draws 0.9954 for the coverage-normalised mean, 0.9885 for the median over the in-frame copies and 0.7499 for the plain
    mean.  The bounds: >= 0.95, >= 0.95, <= 0.80."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts.augmentation_utils import create_augmented_copies
    n, S, s = 100, 128, 32
    yy, xx = np.mgrid[0:S, 0:S]
    obj = (yy > 90) & (xx > 80)
    np.random.seed(1234)
    copies, angles, shifts = create_augmented_copies(obj.astype(F32)[..., None], n, 0.15, 20)
    small = ops.sr_init_target(copies[..., 0].contiguous().view(n, 1, S, S), (s, s))          # the half-pixel bilinear resize
    lr = (small > 0.5).to(torch.float32).cpu().numpy()[..., None]                             # [n, s, s, 1]
    sr = _sr((s, s), (S, S), n, cover="frame")

    def iou(x):
        x = x[..., 0]
        m = x > F32(0.5) * x.max()
        return float((m & obj).sum()) / float((m | obj).sum())

    got = {name: iou(fn(lr, angles, shifts)[0]) for name, fn in (("covered_mean", sr.covered_mean_superresolution),
                                                                  ("covered_median", sr.covered_median_superresolution),
                                                                  ("mean", sr.mean_superresolution))}
    print(f"[realign_covered] corner object IoU: {got}")
    assert got["covered_mean"] >= 0.95
    assert got["covered_median"] >= 0.95
    assert got["mean"] <= 0.80
    cov, none = sr.coverage_map(lr, angles, shifts)
    assert none is None and cov.shape == (S, S, 1) and cov.max() <= n and (cov < n / 2).mean() > 0.05


def test_the_cap(dev, lib):
    """n = cap with the median on 8 x 8 planes (the largest LDS allocation, 160 KiB); cap + 1 with out_median raises and the
    message names the cap; cap + 1 without it returns the rule's mean and coverage."""
    from asr_amd import _lib
    cap = lib.asr_realign_select_max_copies()
    for kind, wgt in (("uniform", "random"), ("mask", "ones")):
        p = _Problem(((8, 8), (8, 8)), "wide", kind, wgt, cap, 1)
        want, got = _rule(p.V, p.C), p.covered()
        for k in want:
            assert np.array_equal(got[k], want[k]), (kind, k)
    p = _Problem(((8, 8), (8, 8)), "trans", "uniform", "random", cap + 1, 1)
    for sub in (("median",), ("mean", "median", "cov")):
        with pytest.raises(_lib.AsrError, match=str(cap)):
            p.covered(want=sub)
    want, got = _rule(p.V, p.C), p.covered(want=("mean", "cov"))
    assert np.array_equal(got["mean"], want["mean"]) and np.array_equal(got["cov"], want["cov"])


# ---- upper layers ---------------------------------------------------------------------------------------------------------
GOLDEN_FILES = {"argmax": ("sr_data_argmax.hdf5", 5, (6, 4), (24, 16)), "slice_max": ("sr_data_slice_max.hdf5", 4, (3, 5), (12, 20))}


def _golden(mode):
    from asr_amd.superresolution_scripts.superres_utils import load_SR_data
    name, n, lr, hr = GOLDEN_FILES[mode]
    return (os.path.join(GOLDEN, name), n, lr, hr) + tuple(load_SR_data(os.path.join(GOLDEN, name), num_aug=n))


def _by_hand(sr, masks, angles, shifts, key):
    """ops.realign_covered's plane for a list of [h, w, 1] copies under cover="frame"."""
    from asr_amd import ops
    yd = ops.to_device(np.asarray(masks)[None, ..., 0])
    rot, tr = sr._transforms(angles[None], shifts[None], yd.device, negate=True)
    ones = torch.ones(yd.shape[2:], dtype=torch.float32, device=yd.device)
    out = ops.realign_covered(yd, ones, tr, rot, sr.output_size, want=(key,), cov_min=sr.cov_min, valid_min=sr.valid_min)
    return out[key][0].cpu().numpy()[..., None]


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_compute_SR_covered_types(dev, tmp_path, mode):
    from asr_amd.superresolution_scripts.superres_utils import compute_SR, threshold_image
    _path, n, lr, hr, masks, max_masks, angles, shifts, name = _golden(mode)
    assert (max_masks is not None) == (mode == "slice_max")
    sr = _sr(lr, hr, n)
    mm = max_masks if max_masks is not None else []
    for t, key in (("covered_mean", "mean"), ("covered_median", "median")):
        got = compute_SR(sr, masks, angles, shifts, name, str(tmp_path), SR_type=t, max_masks=mm, class_id=8, th_factor=0.3,
                         save_final_output=True)
        target = _by_hand(sr, masks, angles, shifts, key)
        method = getattr(sr, f"{t}_superresolution")(masks, angles, shifts)
        assert method[1] is None and method[0].dtype == np.float32 and np.array_equal(method[0], target)
        if mode == "slice_max":                       # the max maps go through the same fusion; class >= max decides
            want = threshold_image(target, 8, th_mask=_by_hand(sr, max_masks, angles, shifts, key))
        else:
            want = threshold_image(target, 8, th_factor=0.3)
        assert got.shape == hr + (1,) and np.array_equal(got, want), t
        assert set(np.unique(got)) <= {0, 8}
        assert (tmp_path / f"{t}_SR" / f"{name}_{t}_SR.png").exists()


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_evaluate_precomputed_covered_types(dev, tmp_path, mode):
    from PIL import Image
    from asr_amd import distributed as D
    from asr_amd.evaluation import evaluate_precomputed
    from asr_amd.superresolution_scripts.superres_utils import compute_SR
    from asr_amd.utils import compute_IoU, load_image
    path, n, lr, hr, masks, max_masks, angles, shifts, name = _golden(mode)
    gt = np.zeros(hr, np.uint8)
    gt[hr[0] // 4:3 * hr[0] // 4, hr[1] // 4:3 * hr[1] // 4] = 8
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    Image.fromarray(gt, mode="L").save(gt_dir / f"{name}.png")
    bad = tmp_path / "9.hdf5"
    bad.write_bytes(b"not an hdf5 file")
    paths = [path, str(bad)]
    kw = dict(num_aug=n, class_id=8, th_factor=0.3, img_size=hr, out_dir=str(tmp_path / "out"))
    table0, valid0 = evaluate_precomputed(_sr(lr, hr, n), paths, str(gt_dir), **kw)
    extra = ("covered_mean", "covered_median")
    res = evaluate_precomputed(_sr(lr, hr, n), paths, str(gt_dir), extra_sr_types=extra, **kw)
    assert len(res) == 3
    table, valid, extras = res
    assert np.array_equal(table, table0, equal_nan=True) and np.array_equal(valid, valid0) and list(valid) == [True, False]
    assert table.shape == (2, len(D.IOU_FIELDS)) and extras.shape == (2, 2) and np.isnan(extras[1]).all()
    sr = _sr(lr, hr, n)
    true_mask = load_image(str(gt_dir / f"{name}.png"), image_size=hr, normalize=False, is_png=True, resize_method="nearest")
    mm = max_masks if max_masks is not None else []
    for j, t in enumerate(extra):
        mask = compute_SR(sr, masks, angles, shifts, name, str(tmp_path / "out"), SR_type=t, max_masks=mm, class_id=8, th_factor=0.3)
        want = compute_IoU(true_mask, mask, img_size=hr, class_id=8)
        assert extras[0, j] == want or (np.isnan(extras[0, j]) and np.isnan(want)), (t, extras[0, j], want)


def test_single_class_script_prints_the_covered_mean(dev, tmp_path):
    from PIL import Image
    from asr_amd.superresolution_scripts import superres_utils as su
    rng = np.random.default_rng(5)
    n, f = 4, 16
    masks = np.zeros((n, f, f, 1), F32)
    masks[:, 4:12, 4:12] = 8.0
    masks += rng.uniform(0, 0.5, masks.shape).astype(F32)
    angles = np.array([0, 0.1, -0.1, 0.05], F32)
    shifts = np.array([[0, 0], [20, -10], [-30, 15], [5, 40]], F32)
    su.save_SR_data(str(tmp_path / "data" / "7"), masks, None, angles, shifts, "7", "argmax", 0.15, 80)
    gt = np.zeros((512, 512), np.uint8)
    gt[128:384, 128:384] = 8
    (tmp_path / "gt").mkdir()
    Image.fromarray(gt, mode="L").save(tmp_path / "gt" / "7.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "SR_single_class.py"), "--data", str(tmp_path / "data"),
                        "--gt", str(tmp_path / "gt"), "--num_aug", str(n), "--class_id", "8", "--feature_size", str(f),
                        "--extra_sr_types", "covered_mean", "--cover", "validity", "--out", str(tmp_path / "out")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    i_ref = next(i for i, l in enumerate(lines) if l.startswith("Avg. Max SR IoUs"))
    extra = [l for l in lines[i_ref + 1:] if l.startswith("Avg. Covered mean SR IoUs: ")]
    assert len(extra) == 1 and 0.0 <= float(extra[0].split(": ")[1]) <= 1.0, r.stdout[-2000:]
    assert (tmp_path / "out" / "covered_mean_SR" / "7_covered_mean_SR.png").exists()


def test_cover_validity(dev):
    """cover="validity" weighs each copy by the part of it that came from inside the image (copy_validity): it differs from
    cover="frame" somewhere on shifted copies and equals it on identity transforms; copy_validity is augment_on_device of an
    all-ones image under the shifts taken to the copies' frame."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts.augmentation_utils import augment_on_device, copy_validity
    n, lr, hr = 6, (16, 24), (64, 96)
    rng = np.random.default_rng(11)
    masks = rng.uniform(0.2, 1.0, (n,) + lr + (1,)).astype(F32)
    angles = rng.uniform(-0.15, 0.15, n).astype(F32)
    shifts = rng.uniform(-20, 20, (n, 2)).astype(F32)
    angles[0], shifts[0] = 0, 0
    val = copy_validity(angles, shifts, hr, lr)
    assert tuple(val.shape) == (n,) + lr and val.dtype == torch.float32 and val.is_cuda
    scaled = (shifts * np.array([lr[1] / hr[1], lr[0] / hr[0]], F32)).astype(F32)
    want = augment_on_device(torch.ones(lr + (1,), dtype=torch.float32, device=dev), angles, scaled)[..., 0]
    assert torch.equal(val, want) and torch.equal(val[0], torch.ones_like(val[0])) and float(val.min()) == 0.0
    assert torch.equal(copy_validity(angles, shifts, lr, lr), augment_on_device(torch.ones(lr + (1,), device=dev), angles, shifts)[..., 0])
    frame, validity = _sr(lr, hr, n, cover="frame"), _sr(lr, hr, n, cover="validity")
    for key, name in (("mean", "covered_mean_superresolution"), ("median", "covered_median_superresolution"), ("cov", "coverage_map")):
        a, b = getattr(frame, name)(masks, angles, shifts)[0], getattr(validity, name)(masks, angles, shifts)[0]
        assert a.shape == b.shape == hr + (1,) and not np.array_equal(a, b), key
        zero_a, zero_s = np.zeros(n, F32), np.zeros((n, 2), F32)
        a, b = getattr(frame, name)(masks, zero_a, zero_s)[0], getattr(validity, name)(masks, zero_a, zero_s)[0]
        assert np.array_equal(a, b), key
    # the batch form: the planes of want, [B, H, W], and the validity weights are those of copy_validity, y weighted by them
    yd = ops.to_device(np.stack([masks[..., 0], masks[::-1, ..., 0]]))
    a2, s2 = np.stack([angles, angles[::-1]]), np.stack([shifts, shifts[::-1]])
    out = validity.realign_covered_batch(yd, a2, s2, ("mean", "cov"))
    assert set(out) == {"mean", "cov"} and tuple(out["mean"].shape) == (2,) + hr
    rot, tr = validity._transforms(a2, s2, dev, negate=True)
    wgt = torch.stack([copy_validity(a2[b], s2[b], hr, lr) for b in range(2)])
    ref = ops.realign_covered((yd * wgt).contiguous(), wgt, tr, rot, hr, want=("mean", "cov"))
    assert torch.equal(out["mean"], ref["mean"]) and torch.equal(out["cov"], ref["cov"])
    assert np.array_equal(out["mean"][0].cpu().numpy()[..., None], validity.covered_mean_superresolution(masks, angles, shifts)[0])
    with pytest.raises(ValueError):
        _sr(lr, hr, n, cover="both")
