"""asr_realign_moments_f32 (csrc/sr.hip: sr_realign_moments_kernel): the mean over the copies that saw a pixel, the population
variance about that rounded mean and the number of those copies, held bit for bit to the rule of include/asr_hip.h.

The yardstick is that of tests/test_gpu_realign_covered.py, whose builders are used here: one asr_realign_max_f32 call on a
stack viewed as [B * n, 1, h, w] folds ONE copy per output plane, so it returns the n warped planes themselves.  Applied once
to y and once to wgt it gives v_i and c_i, and the rule is restated on them in numpy float32: sequential sums in copy order,
the deviation, its square and the add each rounded on their own, one division.  No tolerance anywhere."""
import itertools

import numpy as np
import pytest
import torch

from oracle import tf_ops
from test_gpu_realign_covered import OUT_OF_FRAME, _planes, _transforms

pytestmark = pytest.mark.gpu

SHAPES = (((64, 64), (16, 16)), ((50, 70), (16, 16)),                     # f = 4, a non-multiple with ragged last tiles
          ((3, 33), (2, 9)), ((3, 65), (2, 17)))                            # one live lane / row in the last tiles
MANY = (((8, 8), (4, 4)), 700)                                              # more copies than asr_realign_select_f32 accepts
CASES = ("wide", "trans", "proj")
KINDS = ("uniform", "mask")
WGTS = (None, "ones", "random")
N_ALL = (1, 2, 5, 100)
SUBSETS = [s for r in (1, 2, 3) for s in itertools.combinations(("mean", "var", "nv"), r)]
F32 = np.float32


def _inputs(kind, batch, n, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":                 # signed
        return rng.uniform(-2.0, 2.0, (batch, n, h, w)).astype(F32)
    # {0, c} masks of one object whose edges move by a pixel from copy to copy: plateaus of ties at 0 and at c, c no power of two
    y = np.zeros((batch, n, h, w), F32)
    for b in range(batch):
        c = F32((3.0, 15.0, 0.7)[b % 3])
        for i in range(n):
            t, l = h // 4 + rng.integers(-1, 2), w // 4 + rng.integers(-1, 2)
            y[b, i, t:t + h // 2 + rng.integers(0, 2), l:l + w // 2 + rng.integers(0, 2)] = c
    return y


def _rule(V, Cw, valid_min=0.5):
    """The header's rule on the per-copy planes V, Cw [B, n, H, W] (Cw None: no weight plane) in float32."""
    assert V.dtype == F32 and (Cw is None or Cw.dtype == F32)
    n = V.shape[1]
    valid = np.ones(V.shape, bool) if Cw is None else Cw >= F32(valid_min)
    zero = np.zeros_like(V[:, 0])
    S = zero.copy()
    for i in range(n):                                    # copy order
        S = S + np.where(valid[:, i], V[:, i], F32(0))
    nv = valid.sum(axis=1)
    fnv = nv.astype(F32)
    some = nv > 0
    mean = np.where(some, S / np.where(some, fnv, F32(1)), F32(0)).astype(F32)         # one IEEE division
    s = zero.copy()
    for i in range(n):
        d = V[:, i] - mean
        sq = d * d                                        # rounded on its own ...
        s = s + np.where(valid[:, i], sq, F32(0))         # ... before the add
    assert S.dtype == F32 and s.dtype == F32 and d.dtype == F32 and sq.dtype == F32
    var = np.where(some, s / np.where(some, fnv, F32(1)), F32(0)).astype(F32)
    return {"mean": mean, "var": var, "nv": fnv}


class _Problem:
    def __init__(self, shape, case, kind, wgt, n, batch, seed=210):
        from asr_amd import ops
        (H, W), (h, w) = shape
        self.H, self.W, self.h, self.w, self.n, self.batch = H, W, h, w, n, batch
        self.tag = f"{H}x{W}<-{h}x{w}/{case}/{kind}/{wgt}/n={n}/B={batch}"
        self.y = _inputs(kind, batch, n, h, w, seed)
        self.tr, self.rot, _ang, _sh = _transforms(case, batch, n, H, W, seed + 1)
        self.yd, self.trd, self.rotd = ops.to_device(self.y), ops.to_device(self.tr), ops.to_device(self.rot)
        self.V = _planes(self.yd, self.trd, self.rotd, (H, W))
        if wgt is None:
            self.wd, self.C = None, None
        else:
            if wgt == "ones":
                self.wd = torch.ones((h, w), dtype=torch.float32, device=self.yd.device)
                full = self.wd.expand(batch, n, h, w)
            else:
                self.wd = ops.to_device(np.random.default_rng(seed + 2).uniform(0.0, 1.0, (batch, n, h, w)).astype(F32))
                full = self.wd
            self.C = _planes(full, self.trd, self.rotd, (H, W))
        for a in (self.V, self.C):
            if a is not None:
                assert np.isfinite(a).all()
                a.setflags(write=False)
        if n > OUT_OF_FRAME:
            assert not self.V[:, OUT_OF_FRAME].any()

    def moments(self, want=("mean", "var", "nv"), **kw):
        from asr_amd import ops
        out = ops.realign_moments(self.yd, self.trd, self.rotd, (self.H, self.W), want=want, wgt=self.wd, **kw)
        assert set(out) == set(want)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def check(self, seen):
        from asr_amd import ops
        for kw in (dict(), dict(valid_min=0.25)):
            want, got = _rule(self.V, self.C, **kw), self.moments(**kw)
            for k in ("nv", "mean", "var"):
                assert got[k].shape == (self.batch, self.H, self.W) and got[k].dtype == F32
                assert np.array_equal(got[k], want[k]), (self.tag, kw, k, int((got[k] != want[k]).sum()))
            one, none = want["nv"] == 1, want["nv"] == 0
            assert not got["var"][one].any() and not got["var"][none].any() and not got["mean"][none].any()
            seen["one"] += int(one.sum())
            seen["none"] += int(none.sum())
            seen["spread"] += int((got["var"] > 0).sum())
        full = self.moments()
        again = self.moments()
        for k in full:
            assert full[k].tobytes() == again[k].tobytes(), (self.tag, k)          # two calls: identical bits
        for sub in SUBSETS:
            part = self.moments(want=sub)
            for k in sub:
                assert part[k].tobytes() == full[k].tobytes(), (self.tag, sub, k)
        if self.wd is None:
            plain = ops.realign(self.yd, self.trd, self.rotd, (self.H, self.W), "mean").cpu().numpy()
            assert full["mean"].tobytes() == plain.tobytes(), self.tag               # asr_realign_mean_f32's bits
            assert (full["nv"] == self.n).all()


def _problems(n_index):
    """Every (shape, weight kind) pair for this n; the transform case, the input kind and the batch (1 or 3) rotate with the
    pair and with n, so that over the four n each of them meets every shape and every weight kind."""
    n = N_ALL[n_index]
    for idx, (shape, wgt) in enumerate(itertools.product(SHAPES, WGTS)):
        yield _Problem(shape, CASES[(idx + n_index) % 3], KINDS[(idx // 3 + n_index) % 2], wgt, n, (1, 3)[(idx + n_index) % 2])


@pytest.mark.parametrize("n_index", range(len(N_ALL)), ids=[str(n) for n in N_ALL])
def test_the_rule_bit_for_bit(dev, n_index):
    """out_mean, out_var and out_nv equal the numpy rule on the per-copy planes exactly, at valid_min 0.5 and 0.25, for no
    weight plane, a shared ones plane and per-copy random planes; every non-empty subset of the outputs and a second call
    carry the bits of the full call; without a weight plane out_mean is asr_realign_mean_f32's."""
    seen = dict(one=0, none=0, spread=0)
    for p in _problems(n_index):
        p.check(seen)
    assert seen["spread"] > 0 or N_ALL[n_index] == 1
    if N_ALL[n_index] in (1, 2, 5):
        assert seen["one"] > 0            # pixels that exactly one copy saw do occur: their variance is exactly 0
        assert seen["none"] > 0           # and so do pixels no copy saw (random weights below valid_min, corners out of frame)


@pytest.mark.parametrize("kind,wgt", [("uniform", "random"), ("mask", None), ("mask", "ones")])
def test_more_copies_than_the_select_cap(dev, lib, kind, wgt):
    """n = 700 on 8 x 8 <- 4 x 4: above asr_realign_select_max_copies(), no cap here."""
    shape, n = MANY
    assert n > lib.asr_realign_select_max_copies()
    seen = dict(one=0, none=0, spread=0)
    _Problem(shape, "trans", kind, wgt, n, 1).check(seen)
    assert seen["spread"] > 0


def test_nobody_saw_it(dev):
    """Every copy shifted out of frame by +-W under a weight plane: mean, variance and count are 0 everywhere.  With one copy
    left in place the count is 1 where it is in frame, the mean is that copy's plane there and the variance exactly 0.
    Without a weight plane the same copies all count, as zeros."""
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
        out = ops.realign_moments(yd, tr, rot, (H, W), want=("mean", "var", "nv"), wgt=wd)
        return {k: v.cpu().numpy() for k, v in out.items()}, _planes(yd, tr, rot, (H, W))

    for wd in (ones, rnd):
        out, _ = run(sh, wd)
        for k, v in out.items():
            assert not v.any(), k
    out, _ = run(sh, None)
    assert (out["nv"] == n).all() and not out["mean"].any() and not out["var"].any()
    sh2 = sh.copy()
    sh2[:, 4] = [7.0, -3.0]                                  # copy 4 stays (partly) in frame
    out, V = run(sh2, ones)
    assert set(np.unique(out["nv"])) == {0.0, 1.0}
    alone = out["nv"] == 1
    assert np.array_equal(out["mean"][alone], V[:, 4][alone]) and not out["mean"][~alone].any()
    assert not out["var"].any()
    out, V = run(sh2, None)                                  # five zeros and copy 4: a spread wherever copy 4 is not 0
    assert (out["nv"] == n).all() and np.array_equal(out["var"] > 0, V[:, 4] != 0)


def test_superresolution_surface(dev):
    """variance_superresolution and realign_moments_batch are ops.realign_moments under the object's cover and valid_min;
    cover=None passes no weight plane, and its mean is mean_superresolution's."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts.augmentation_utils import copy_validity
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    n, lr, hr = 6, (16, 24), (64, 96)
    rng = np.random.default_rng(11)
    masks = rng.uniform(0.2, 1.0, (n,) + lr + (1,)).astype(F32)
    angles = rng.uniform(-0.15, 0.15, n).astype(F32)
    shifts = rng.uniform(-20, 20, (n, 2)).astype(F32)
    yd = ops.to_device(masks[None, ..., 0])
    made = {}
    for cover, valid_min in (("frame", 0.5), ("validity", 0.25)):
        sr = Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=3, num_aug=n, feature_size=lr, output_size=hr, cover=cover,
                             valid_min=valid_min)
        rot, tr = sr._transforms(angles[None], shifts[None], dev, negate=True)
        wgt = torch.ones(lr, dtype=torch.float32, device=dev) if cover == "frame" else \
            copy_validity(angles, shifts, hr, lr)[None].contiguous()
        want = ops.realign_moments(yd, tr, rot, hr, want=("mean", "var", "nv"), wgt=wgt, valid_min=valid_min)
        got = sr.realign_moments_batch(yd, angles[None], shifts[None], ("mean", "var", "nv"))
        for k in want:
            assert torch.equal(got[k], want[k]), (cover, k)
        var, none = sr.variance_superresolution(masks, angles, shifts)
        assert none is None and var.shape == hr + (1,) and var.dtype == F32
        assert np.array_equal(var[..., 0], want["var"][0].cpu().numpy()) and var.max() > 0
        made[cover] = var
        bare = sr.realign_moments_batch(yd, angles[None], shifts[None], ("mean", "nv"), cover=None)
        assert np.array_equal(bare["mean"][0].cpu().numpy()[..., None], sr.mean_superresolution(masks, angles, shifts)[0])
        assert (bare["nv"] == n).all()
    assert not np.array_equal(made["frame"], made["validity"])
