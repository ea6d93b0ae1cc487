"""The windowed CRF (asr_crf_unaries_* / asr_crf_refine_f32, ops.crf_*) against tests/crf_ref.py, a numpy restatement of the
rule in include/asr_hip.h that is never the library.

Error scale.  It is not fixed in advance: e32 = max |Q(float32 restatement) - Q(float64 restatement)| on the same inputs, and
the library's Q must stay within tol = max(8 * e32, 2^-18) of the float64 Q.  The 8 allows another summation and another exp
path; it is not a measurement of the kernel.  Labels must equal the float64 argmax wherever the float64 top-two margin of the
final logits exceeds 2 * tol, and at most 1 % of a case's pixels may be excluded that way.  Every accuracy check prints its
e_gpu / e32 and its excluded share before it asserts."""
import zlib

import numpy as np
import pytest
import torch

import crf_ref

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -18
TH, TAU = 0.15, 0.1
# (H, W, K, r, d)
CASES = [(37, 70, 3, 3, 1), (40, 72, 20, 2, 2), (3, 65, 2, 4, 1), (65, 3, 2, 4, 1), (33, 33, 1, 5, 1),
         (40, 72, 2, 4, 4),             # halo 16: wider than half a tile
         (34, 34, 31, 1, 1),            # L at its cap
         (1, 1, 2, 1, 1)]
ITERATIONS = (0, 1, 5)
_CACHE = {}


def make_guide(kind, H, W, rng):
    if kind == "uniform":
        return rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    Y, X = np.mgrid[0:H, 0:W]                              # two colours, a slanted edge
    colours = np.array([[0.8, 0.3, 0.2], [0.2, 0.5, 0.7]], dtype=np.float32)
    return colours[(2 * Y + X >= (2 * H + W) // 2).astype(int)]


def class_ids(K):
    return list(range(1, K + 1))


def case(shape, kind, T, **extra):
    """Inputs and both restatements of one case, computed once and shared (never modified): guide, scores, z (the numpy f32
    unaries), s64, Q64, e32."""
    key = (shape, kind, T, tuple(sorted(extra.items())))
    if key not in _CACHE:
        H, W, K, r, d = shape
        rng = np.random.default_rng(zlib.crc32(repr((shape, kind)).encode()))
        guide = make_guide(kind, H, W, rng)
        scores = rng.uniform(0.0, 1.0, (K, H, W)).astype(np.float32)
        z = crf_ref.unaries_scores(scores, TH, TAU)
        prm = dict(radius=r, dilation=d, iterations=T, **extra)
        s64, q64 = crf_ref.crf(guide, z, np.float64, **prm)
        e32 = float(np.abs(crf_ref.crf(guide, z, np.float32, **prm)[1].astype(np.float64) - q64).max())
        for a in (guide, scores, z, s64, q64):
            a.setflags(write=False)
        _CACHE[key] = (guide, scores, z, s64, q64, e32)
    return _CACHE[key]


def run(dev, guide, z, ids, want_q=True, **params):
    from asr_amd import ops
    out = ops.crf_refine(torch.tensor(guide).to(dev), torch.tensor(z).to(dev), ids, params, want_q=want_q)
    if want_q:
        return out[0].cpu().numpy(), out[1].cpu().numpy()
    return out.cpu().numpy()


def check_against(name, labels, q, s64, q64, e32, ids):
    tol = max(8.0 * e32, FLOOR)
    e_gpu = float(np.abs(q.astype(np.float64) - q64).max())
    sure = crf_ref.top_two_margin(s64) > 2.0 * tol
    excluded = 1.0 - float(sure.mean())
    wrong = int((labels != crf_ref.labels_of(s64, ids))[sure].sum())
    print(f"crf {name}: e_gpu {e_gpu:.3e}  e32 {e32:.3e}  e_gpu/e32 {e_gpu / e32 if e32 else float('inf'):.3f}  tol {tol:.3e}  "
          f"excluded {100 * excluded:.4f} %  wrong labels {wrong}  sum-1 {float(np.abs(q.sum(axis=0, dtype=np.float64) - 1).max()):.2e}")
    assert q.dtype == np.float32 and labels.dtype == np.int32 and np.isfinite(q).all()
    assert e_gpu <= tol
    assert excluded <= 0.01
    assert wrong == 0
    assert np.abs(q.sum(axis=0, dtype=np.float64) - 1.0).max() <= 1e-6


# ---- accuracy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", ITERATIONS)
@pytest.mark.parametrize("kind", ["uniform", "two_colour"])
@pytest.mark.parametrize("shape", CASES)
def test_matches_the_float64_restatement(dev, shape, kind, T):
    guide, _, z, s64, q64, e32 = case(shape, kind, T)
    H, W, K, r, d = shape
    labels, q = run(dev, guide, z, class_ids(K), radius=r, dilation=d, iterations=T)
    assert labels.shape == (H, W) and q.shape == (K + 1, H, W)
    check_against(f"{H}x{W} K={K} r={r} d={d} T={T} {kind}", labels, q, s64, q64, e32, class_ids(K))


def test_the_exponent_clamp_stays_within_the_tolerance(dev):
    """One pixel of colour 1 in an all-0 image at theta_rgb = 0.05: |I_p - I_q|^2 / (2 theta^2) = 600, so the exponent is below
    -600, far beyond -80: the clamp acts on every weight between the bright pixel and its neighbours."""
    shape, ids = (37, 70, 3, 3, 1), class_ids(3)
    _, _, z, _, _, _ = case(shape, "uniform", 5)
    guide = np.zeros((37, 70, 3), dtype=np.float32)
    guide[17, 40] = 1.0
    prm = dict(radius=3, dilation=1, iterations=5, theta_rgb=0.05)
    s64, q64 = crf_ref.crf(guide, z, np.float64, **prm)
    e32 = float(np.abs(crf_ref.crf(guide, z, np.float32, **prm)[1].astype(np.float64) - q64).max())
    labels, q = run(dev, guide, z, ids, **prm)
    check_against("37x70 K=3 one bright pixel theta_rgb=0.05", labels, q, s64, q64, e32, ids)


# ---- properties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(37, 70, 3, 3, 1), (40, 72, 20, 2, 2), (40, 72, 2, 4, 4)])
def test_repeatable_and_want_q_changes_no_label(dev, shape):
    from asr_amd import ops
    guide, _, z, _, _, _ = case(shape, "uniform", 5)
    H, W, K, r, d = shape
    g, zt, prm = torch.tensor(guide).to(dev), torch.tensor(z).to(dev), dict(radius=r, dilation=d, iterations=5)
    l1, q1 = ops.crf_refine(g, zt, class_ids(K), prm, want_q=True)
    l2, q2 = ops.crf_refine(g, zt, class_ids(K), prm, want_q=True)
    assert torch.equal(l1, l2) and torch.equal(q1, q2)                         # two identical calls, the same bits
    out = torch.full((H, W), -7, dtype=torch.int32, device=dev)
    assert ops.crf_refine(g, zt, class_ids(K), prm, out=out) is out
    assert torch.equal(out, l1)                                                # the labels do not depend on want_q


def test_zero_iterations_at_one_class_is_the_fusion(dev):
    from asr_amd import ops
    guide, scores, _, _, _, _ = case((33, 33, 1, 5, 1), "uniform", 0)
    s = torch.tensor(scores).to(dev)
    fused, _ = ops.fuse_labels(s, [8], th_factor=TH)
    labels = ops.crf_refine(torch.tensor(guide).to(dev), ops.crf_unaries(s, TH, TAU), [8], dict(iterations=0, radius=5))
    assert torch.equal(labels, fused)
    assert 0 < int((fused == 8).sum()) < fused.numel()


def test_zero_iterations_where_one_class_passes_is_the_fusion(dev):
    from asr_amd import ops
    H, W, ids = 37, 70, [3, 9, 15]
    rng = np.random.default_rng(77)
    winner = rng.integers(0, 4, (H, W))                                        # 0: no class passes
    scores = rng.uniform(0.0, 0.1, (3, H, W)).astype(np.float32)
    for k in range(3):
        scores[k][winner == k + 1] = rng.uniform(0.5, 1.0, int((winner == k + 1).sum())).astype(np.float32)
    assert all(TH * scores[k].max() > 0.1 for k in range(3))                   # the losers stay below every threshold
    s = torch.tensor(scores).to(dev)
    fused, _ = ops.fuse_labels(s, ids, th_factor=TH)
    guide = torch.tensor(make_guide("uniform", H, W, rng)).to(dev)
    labels = ops.crf_refine(guide, ops.crf_unaries(s, TH, TAU), ids, dict(iterations=0))
    assert torch.equal(labels, fused)
    assert np.array_equal(fused.cpu().numpy(), np.concatenate([[0], ids])[winner])


def test_zero_weights_leave_the_softmax_of_the_unaries(dev):
    """"Q is bitwise the softmax of z" is read as: bitwise the library's own Q^0 (the T = 0 call), since with zero weights every
    iteration's logits are z exactly.  Q^0 itself is an f32 softmax and is held against the float64 one to 2^-18 only."""
    from asr_amd import ops
    guide, _, z, _, _, _ = case((37, 70, 3, 3, 1), "uniform", 5)
    g, zt, ids = torch.tensor(guide).to(dev), torch.tensor(z).to(dev), class_ids(3)
    l0, q0 = ops.crf_refine(g, zt, ids, dict(iterations=0), want_q=True)
    l5, q5 = ops.crf_refine(g, zt, ids, dict(iterations=5, w_app=0.0, w_smooth=0.0), want_q=True)
    assert torch.equal(l5, l0) and torch.equal(q5, q0)
    soft = crf_ref.softmax(z.astype(np.float64))
    assert np.abs(q0.cpu().numpy() - soft).max() <= FLOOR


def test_both_unary_kernels_are_bitwise_their_numpy_restatement(dev):
    from asr_amd import ops
    _, scores, z, _, _, _ = case((40, 72, 20, 2, 2), "uniform", 0)
    got = ops.crf_unaries(torch.tensor(scores).to(dev), TH, TAU).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), z.view(np.uint32))
    rng = np.random.default_rng(5)
    ids = [2, 5, 7, 19]
    labels = rng.choice(np.array([0, 2, 5, 7, 19, 255, 3], dtype=np.int32), (37, 70))
    for conf in (0.7, 0.21, 0.999):
        got = ops.crf_unaries_from_labels(torch.tensor(labels).to(dev), ids, conf).cpu().numpy()
        want = crf_ref.unaries_labels(labels, ids, conf)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), conf
    assert (want[:, labels == 255] == 0).all() and (want[:, labels == 3] == 0).all()


# ---- what it is for ------------------------------------------------------------------------------------------------------
def test_it_moves_an_upsampled_boundary_onto_the_image_edge(dev):
    from asr_amd import ops
    from test_gpu_guided_filter import iou, synthetic_object
    mask, guide, p, near = synthetic_object()
    g, s = torch.tensor(guide).to(dev), torch.tensor(p[None]).to(dev)
    z = ops.crf_unaries(s, 0.5, TAU)
    raw = ops.crf_refine(g, z, [1], dict(iterations=0)).cpu().numpy() == 1
    assert np.array_equal(raw, ops.fuse_labels(s, [1], th_factor=0.5)[0].cpu().numpy() == 1)
    refined = ops.crf_refine(g, z, [1]).cpu().numpy() == 1                     # the defaults
    ref = crf_ref.labels_of(crf_ref.crf(guide, crf_ref.unaries_scores(p[None], 0.5, TAU))[0], [1]) == 1
    before, after = iou(raw, mask), iou(refined, mask)
    print(f"crf synthetic object: IoU {before:.4f} -> {after:.4f} (float64 {iou(ref, mask):.4f}); within 2 px "
          f"{iou(raw, mask, near):.4f} -> {iou(refined, mask, near):.4f}")
    assert before <= 0.97 and after >= 0.99
