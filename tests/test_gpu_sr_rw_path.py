"""Copy reweighting in the upper layers, on the small model input of the label-map path tests: Superresolution(reweight=...),
compute_SR, HotPath.run_image_labels(sr_reweight=...), evaluate_labelmaps and scripts/validate_labelmap.py return the weights
ops.sr_solve returns for the same stacks; nothing changes without the keyword; the copy-weights CSV round-trips; the scripts' flags reach the solve."""
import csv
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_labelmap_path import ANGLE, ITERS, N_AUG, REQ, SCRIPT, SHIFT, TH, _dataset, _run, _sr, _weights

sys.path.insert(0, GOLDEN)
from make_hotpath_traces import small_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

SR_KEYS = ("aug", "max", "mean")
NUM_ITER = 12
RW = dict(kind="cauchy", kappa=1.0, every=3, start=2)        # reweights at 2, 5, 8, 11 of the 12 iterations


@pytest.fixture(scope="module")
def small(dev):
    return small_inputs(dev)


def _labels(small, mode, **kw):
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    sr = _sr("adam", 6, NUM_ITER, (16, 16), (64, 64), False)
    sr.optimizer.optimizer.iterations = 123
    starts = {c: 7 * j + 2 for j, c in enumerate(REQ)}
    path = HotPath(model, sr, mode=mode, th_factor=TH, batch_size=4)
    return path.run_image_labels(img, angles, shifts, REQ, gt_dev=gt, adam_starts=starts, **kw), starts, path


def _same(res, ref, extra=(), keys=("standard",) + SR_KEYS):
    assert sorted(res) == sorted(list(ref) + list(extra)) and res["solved_ids"] == ref["solved_ids"]
    for key in keys:
        assert torch.equal(res[key], ref[key]), key
        assert np.array_equal(res["counts"][key], ref["counts"][key]), key


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_the_path_returns_the_weights_of_the_class_solve(small, mode):
    from asr_amd import ops
    _, img, gt, angles, shifts = small
    plain, _, p0 = _labels(small, mode)
    none, _, _ = _labels(small, mode, sr_reweight=None)
    assert "copy_weights" not in plain and "copy_weights" not in none
    _same(none, plain)
    res, starts, path = _labels(small, mode, sr_reweight=RW, keep_scores=True, coverages=[100], keep_uncertainty=True)
    solved, stacks = res["solved_ids"], res["uncertainty_stacks"]
    cw = res["copy_weights"]
    print(mode, {k: v.round(3).tolist() for k, v in cw.items()})
    assert sorted(cw) == (["aug", "aug_max"] if mode == "slice_max" else ["aug"])
    for v in cw.values():
        assert v.dtype == np.float32 and v.shape == (len(solved), 6) and (v >= 0).all() and (v <= 1).all() and (v < 1).any()
    assert path.sr.reweight is None                                       # the shared solver object is left as it was
    assert path.sr.optimizer.optimizer.iterations == p0.sr.optimizer.optimizer.iterations
    for t in ("standard", "max", "mean"):
        assert torch.equal(res[t], plain[t])
    no_aug, _, _ = _labels(small, mode, sr_types=("max", "mean"), sr_reweight="hard")
    assert no_aug["copy_weights"] == {}
    if mode != "argmax":
        return                      # (the stacks kept for the uncertainty are the argmax path's solver input as they are)
    fshifts = path._sr_frame(img, shifts)
    sr = _sr("adam", 6, NUM_ITER, (16, 16), (64, 64), False)
    sr.reweight = ops.check_sr_reweight(dict(RW, history=False))
    scores = sr.augmented_superresolution_classes(stacks, angles, fshifts, [starts[c] for c in solved])[0]
    assert np.array_equal(sr.last_copy_weights.weights.cpu().numpy().view(np.uint32), cw["aug"].view(np.uint32))
    assert torch.equal(scores, res["scores"]["aug"][0])
    # the reweighting did something, and a later unreweighted solve of the same object forgets the weights
    sr.reweight = None
    plain_scores = sr.augmented_superresolution_classes(stacks, angles, fshifts, [starts[c] for c in solved])[0]
    assert sr.last_copy_weights is None and not torch.equal(plain_scores, scores)


def test_superresolution_reweight_is_the_ops_solve(dev):
    """Superresolution(reweight=...) through augmented_superresolution gives ops.sr_solve's weights and result."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    import sr_dt_ref as RD
    case = RD.make_case(0, H=32, h=8, n=8, n_bad=2)
    kw = dict(reweight="hard", reweight_kappa=2.0, reweight_every=2, reweight_start=1)
    sr = _sr("adam", 8, 6, (8, 8), (32, 32), False)
    ref = _sr("adam", 8, 6, (8, 8), (32, 32), False)
    sr.reweight = Superresolution.check_reweight(**kw)
    x, loss = sr.augmented_superresolution(case["copies"][..., None], case["angles"], case["shifts"])
    x0, _ = ref.augmented_superresolution(case["copies"][..., None], case["angles"], case["shifts"])
    cw = sr.last_copy_weights
    assert tuple(cw.weights.shape) == (1, 8) and cw.history is None and cw.iters == [1, 3, 5]
    assert ref.last_copy_weights is None and not np.array_equal(x, x0) and np.isfinite(loss)
    # the same solve by hand
    y = ops.to_device(case["copies"][None])
    rot, tr = ref._transforms(case["angles"][None], case["shifts"][None], y.device)
    irot, itr = ref._transforms(case["angles"][None], case["shifts"][None], y.device, inverse=True)
    opt = _sr("adam", 8, 6, (8, 8), (32, 32), False).optimizer
    alphas = ops.to_device(np.stack([opt.schedule_alphas(6)], axis=1))
    out = ops.sr_solve(ops.sr_init_target(y, (32, 32)), y, rot, tr, irot, itr, alphas, ref._lambdas,
                       cfg=opt.optimizer.config(use_btv=False), slot_init=opt.optimizer.slot_init,
                       reweight=dict(kind="hard", kappa=2.0, every=2, start=1))
    assert torch.equal(out[2].weights, cw.weights) and np.array_equal(out[0][0].cpu().numpy(), x[..., 0])
    with pytest.raises(ValueError, match="verbose"):
        Superresolution(1, 0.3, 0, 0, num_iter=2, num_aug=2, feature_size=(4, 4), output_size=(8, 8), verbose=True, reweight="hard")


def test_the_copy_weights_csv_round_trips(tmp_path):
    from asr_amd.evaluation import read_copy_weights_csv, write_copy_weights_csv
    rows = [("2007_000033", "1", 0, np.float32(0.1)), ("2007_000033", "15_max", 7, 1.0), ("a,b \"c\"", "3", 2, np.float32(1e-30))]
    p = str(tmp_path / "cw.csv")
    write_copy_weights_csv(p, rows)
    got = read_copy_weights_csv(p)
    assert [(a, b, c) for a, b, c, _ in got] == [(a, b, c) for a, b, c, _ in rows]
    assert [np.float32(w).tobytes() for *_, w in got] == [np.float32(w).tobytes() for *_, w in rows]
    open(p, "w").write("x,y\n")
    with pytest.raises(ValueError, match="not a copy-weights CSV"):
        read_copy_weights_csv(p)


def test_validate_labelmap_script_writes_the_copy_weights(dev, tmp_path):
    from asr_amd.evaluation import read_copy_weights_csv
    root = str(tmp_path)
    img_dir, gt_dir = _dataset(root)
    weights = _weights(root, dev)
    out, cw = os.path.join(root, "rw.csv"), os.path.join(root, "cw.csv")
    base = [sys.executable, SCRIPT, "--images", img_dir, "--gt", gt_dir, "--num_aug", str(N_AUG), "--num_iter", str(ITERS),
            "--mode", "argmax", "--angle_max", str(ANGLE), "--shift_max", str(SHIFT), "--th_factor", str(TH), "--weights", weights,
            "--no_prune"]
    _run(base + ["--out", out, "--sr_reweight", "cauchy", "--sr_reweight_kappa", "1", "--sr_reweight_every", "2",
                 "--sr_reweight_start", "1", "--copy_weights_out", cw])
    with open(out, newline="") as fh:
        assert list(csv.reader(fh))[0] == ["Name", "standard_iou", "aug_iou", "max_iou", "mean_iou", "n"]
    got = read_copy_weights_csv(cw)
    images = sorted(os.path.splitext(f)[0] for f in os.listdir(img_dir))
    classes = sorted({c for _, c, _, _ in got}, key=int)
    assert len(classes) >= 2 and len(got) == len(images) * len(classes) * N_AUG        # one row per image, class and copy
    assert sorted({i for i, *_ in got}) == images and sorted({k for *_, k, _ in got}) == list(range(N_AUG))
    assert all(0.0 <= w <= 1.0 for *_, w in got) and any(w < 1.0 for *_, w in got)


# ---- the batch and class entry points against ops.sr_solve -------------------------------------------------------------------------
def _by_ops(sr, y, angles, shifts, alphas, reweight, **kw):
    """ops.sr_solve on the stacks y [B,N,h,w] with the object's transforms, lambdas and update rule -> its return value."""
    from asr_amd import ops
    rot, tr = sr._transforms(angles, shifts, y.device)
    irot, itr = sr._transforms(angles, shifts, y.device, inverse=True)
    state = sr.optimizer.optimizer
    return ops.sr_solve(ops.sr_init_target(y, sr.output_size), y, rot, tr, irot, itr, alphas, sr._lambdas,
                        cfg=state.config(use_btv=False), slot_init=state.slot_init, reweight=reweight, **kw)


def test_the_batch_and_the_coupled_class_solve_return_the_weights_of_ops_sr_solve(dev):
    from asr_amd import ops
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    import sr_dt_ref as RD
    rw = dict(kind="cauchy", kappa=2.0, every=2, start=1)
    cases = [RD.make_case(s, H=32, h=8, n=8, n_bad=2) for s in (0, 1)]
    y = ops.to_device(np.stack([c["copies"] for c in cases]))
    angles, shifts = np.stack([c["angles"] for c in cases]), np.stack([c["shifts"] for c in cases])
    # augmented_superresolution_batch: two images, the Adam counter advancing image by image
    sr = _sr("adam", 8, 6, (8, 8), (32, 32), False)
    sr.reweight = Superresolution.check_reweight("cauchy", 2.0, 2, 1)
    x, _ = sr.augmented_superresolution_batch(y, angles, shifts)
    opt = _sr("adam", 8, 6, (8, 8), (32, 32), False).optimizer
    alphas = ops.to_device(np.stack([opt.schedule_alphas(6) for _ in range(2)], axis=1))
    out = _by_ops(sr, y, angles, shifts, alphas, rw)
    assert torch.equal(out[0], x) and torch.equal(out[2].weights.view(torch.int32), sr.last_copy_weights.weights.view(torch.int32))
    assert tuple(sr.last_copy_weights.weights.shape) == (2, 8) and bool((sr.last_copy_weights.weights < 1).any())
    # augmented_superresolution_classes(couple=True): two classes of one image in one coupled primal-dual solve
    def pd():
        return Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=6, num_aug=8, optimizer=Optimizer("primal_dual"), feature_size=(8, 8),
                               output_size=(32, 32), reweight="cauchy", reweight_kappa=2.0, reweight_every=2, reweight_start=1)
    stacks = ops.to_device(np.stack([cases[0]["copies"], 1.0 - cases[0]["copies"]]))
    a1, s1 = cases[0]["angles"], cases[0]["shifts"]
    srp = pd()
    xc, _ = srp.augmented_superresolution_classes(stacks, a1, s1, [0, 6], couple=True)
    cwc = srp.last_copy_weights.weights
    a2, s2 = np.repeat(a1[None], 2, axis=0), np.repeat(s1[None], 2, axis=0)
    rot, tr = srp._transforms(a2, s2, dev)
    irot, itr = srp._transforms(a2, s2, dev, inverse=True)
    state = srp.optimizer.optimizer
    bound = ops.sr_data_bound(rot, tr, irot, itr, (32, 32), (8, 8), 1.0, iters=state.bound_iters)
    outc = ops.sr_solve(ops.sr_init_target(stacks, (32, 32)), stacks, rot, tr, irot, itr, ops.pd_steps(bound, 0.7, 6), srp._lambdas,
                        cfg=state.config(use_btv=False), slot_init=state.slot_init, reweight=rw, coupling=2)
    assert torch.equal(outc[0], xc) and torch.equal(outc[2].weights.view(torch.int32), cwc.view(torch.int32))
    sru = pd()
    xu, _ = sru.augmented_superresolution_classes(stacks, a1, s1, [0, 6])
    assert not torch.equal(xu, xc) and tuple(cwc.shape) == (2, 8)


# ---- compute_SR ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_max", [False, True])
def test_compute_SR_with_a_reweighting_solver(dev, tmp_path, with_max):
    """compute_SR(SR_type="aug") with a Superresolution(reweight=...) on the construction of sr_dt_ref (5 of 20 copies replaced,
    150 AMSGrad iterations), without and with max_masks: the mask is the threshold of the object's own solves, last_copy_weights
    (of the solve compute_SR ran last: the class map's, or the max map's) equals ops.sr_solve's bit for bit, and the mask
    differs from the unreweighted one -- there the replaced copies still pull."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    from asr_amd.superresolution_scripts.superres_utils import compute_SR, threshold_image
    import sr_dt_ref as RD
    case = RD.make_case(0)
    n, h, H = RD.N_COPIES, RD.H_LR, RD.H_HR
    masks = list(case["copies"][..., None])
    max_masks = [np.float32(0.5) * m + np.float32(0.2) for m in masks] if with_max else []       # another stack, as slice_max's
    angles, shifts = case["angles"], case["shifts"]
    rw = dict(kind="hard", kappa=2.0, every=10, start=10)

    def fresh(**k):                                                           # a fresh Adam counter for every object
        return Superresolution(*RD.LAMBDAS, num_iter=RD.ITERS, num_aug=n, optimizer=Optimizer("adam", RD.LR, amsgrad=True),
                               feature_size=(h, h), output_size=(H, H), **k)
    kw = dict(reweight="hard", reweight_kappa=2.0, reweight_every=10, reweight_start=10)
    sr = fresh(**kw)
    got = compute_SR(sr, masks, angles, shifts, "case0", str(tmp_path), SR_type="aug", max_masks=max_masks, class_id=8, th_factor=0.5)
    last = sr.last_copy_weights.weights
    assert tuple(last.shape) == (1, n) and bool((last < 1).any())
    # the same by hand: the object's solves, then ops.sr_solve for the solve compute_SR ran last
    ref = fresh(**kw)
    target = ref.augmented_superresolution(masks, angles, shifts)[0]
    t_max = ref.augmented_superresolution(max_masks, angles, shifts)[0] if with_max else None
    want = threshold_image(target, 8, th_mask=t_max) if with_max else threshold_image(target, 8, th_factor=0.5)
    assert np.array_equal(got, want)
    opt = fresh().optimizer
    for stack in [masks] + ([max_masks] if with_max else []):
        alphas = ops.to_device(np.stack([opt.schedule_alphas(RD.ITERS)], axis=1))            # the counter runs on from solve to solve
        y = ops.to_device(np.asarray(stack, dtype=np.float32)[None, ..., 0])
        out = _by_ops(ref, y, angles[None], shifts[None], alphas, rw)
    assert torch.equal(out[2].weights.view(torch.int32), last.view(torch.int32))
    assert np.array_equal(out[0][0].cpu().numpy()[..., None], t_max if with_max else target)
    if not with_max:                                                          # the hard weights found exactly the replaced copies
        cw = last.cpu().numpy()[0]
        assert (cw[case["bad"]] == 0).all() and (np.delete(cw, case["bad"]) == 1).all()
    plain = compute_SR(fresh(), masks, angles, shifts, "case0", str(tmp_path), SR_type="aug", max_masks=max_masks, class_id=8,
                       th_factor=0.5)
    assert not np.array_equal(plain, got)


# ---- evaluate_labelmaps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_evaluate_labelmaps_rows_are_run_image_labels_weights(small, tmp_path, mode):
    """evaluate_labelmaps(sr_reweight=, copy_weights=[]) in process: its rows, after a CSV round trip, are bit for bit the
    "copy_weights" of run_image_labels for the same image, draws and Adam starts -- class by class, copy by copy, the max maps'
    solve under "<id>_max"; without the keyword (or with None passed) the results and the label-map CSV are the run before's."""
    from PIL import Image
    from bench import synth_image
    from asr_amd import distributed as D, evaluation as E
    from asr_amd.pipeline import HotPath
    model, _, gt, _, _ = small
    images, gts = [], []
    for g in range(2):
        arr = synth_image(np.random.default_rng(21 + g), 64)
        images.append(str(tmp_path / f"im{g}.png"))
        Image.fromarray(np.clip(np.rint(arr * 255.0), 0, 255).astype(np.uint8), mode="RGB").save(images[-1])
        lab = gt.cpu().numpy().astype(np.uint8)
        gts.append(str(tmp_path / f"gt{g}.png"))
        Image.fromarray(lab if g == 0 else lab[::-1].copy(), mode="L").save(gts[-1])
    path = lambda: HotPath(model, _sr("adam", 6, NUM_ITER, (16, 16), (64, 64), False), mode=mode, th_factor=TH, batch_size=4)
    kw = dict(num_aug=6, angle_max=0.15, shift_max=8, img_size=(64, 64))
    run = lambda **k: E.evaluate_labelmaps(path(), images, gts, REQ, **kw, **k)
    rows = []
    ref, none, out = run(), run(sr_reweight=None, copy_weights=None), run(sr_reweight=RW, copy_weights=rows)
    # without the keyword: the same results and the same CSV, byte for byte
    assert np.array_equal(none.rows, ref.rows, equal_nan=True) and np.array_equal(none.counts, ref.counts) and len(none) == len(ref) == len(out)
    csvs = []
    for tag, res in (("ref", ref), ("none", none)):
        csvs.append(str(tmp_path / f"{tag}.csv"))
        E.write_labelmap_csv(csvs[-1], res.counts, res.rows)
    assert open(csvs[0], "rb").read() == open(csvs[1], "rb").read()
    for j in (0, 2, 3):                                                      # standard, max, mean: the solver option is not theirs
        assert np.array_equal(out.counts[j], ref.counts[j])
    # the rows through the CSV
    p = str(tmp_path / "cw.csv")
    E.write_copy_weights_csv(p, rows)
    got = E.read_copy_weights_csv(p)
    assert [(a, b, c, np.float32(w).tobytes()) for a, b, c, w in got] == [(a, b, c, np.float32(w).tobytes()) for a, b, c, w in rows]
    # the same images through run_image_labels, with evaluate_labelmaps' own draws and Adam starts
    class_ids, params, mine = E._class_set_run(REQ, images, gts, 0, 1, num_aug=6, angle_max=0.15, shift_max=8, seed=1234)
    hp = path()
    starts = D.adam_class_starts(np.ones((2, len(class_ids)), dtype=bool), hp.sr.num_iter, mode)
    want = []
    for g in mine:
        image, lab = E._image_and_labels_on_device(images[g], gts[g], (64, 64))
        res = hp.run_image_labels(image, *params[g], class_ids, gt_dev=lab, sr_reweight=RW,
                                  adam_starts={c: int(starts[g, k]) for k, c in enumerate(class_ids)})
        assert sorted(res["copy_weights"]) == (["aug", "aug_max"] if mode == "slice_max" else ["aug"])
        for solve in sorted(res["copy_weights"]):
            for c, row in zip(res["solved_ids"], res["copy_weights"][solve]):
                want += [(f"im{g}", f"{c}_max" if solve == "aug_max" else str(c), i, np.float32(v).tobytes()) for i, v in enumerate(row)]
    assert len(want) > 0 and [(a, b, c, np.float32(w).tobytes()) for a, b, c, w in got] == want
    assert any(np.frombuffer(w, np.float32)[0] < 1 for *_, w in want)
    if mode == "slice_max":
        assert any(b.endswith("_max") for _, b, _, _ in want)
        a_rows = [w for _, b, _, w in want if not b.endswith("_max")]
        m_rows = [w for _, b, _, w in want if b.endswith("_max")]
        assert len(a_rows) == len(m_rows) and a_rows != m_rows              # a swapped tag would not go unseen
