"""GPU: the data term through the upper layers -- Superresolution(df_loss=...), df_weights= on the solves, compute_SR, and
HotPath.run_image_labels(df_weights="maxprob" | "margin") -- on the small model of the label-map path tests."""
import numpy as np
import pytest
import torch

from test_gpu_sr_wtv import _upper, SR_KEYS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small(dev):
    return _upper()[1](dev)


def _sr(n=6, iters=5, feat=(16, 16), out=(64, 64), **kw):
    """test_gpu_labelmap_path._sr("adam", ...) with the data-term keywords."""
    from asr_amd.superresolution_scripts.optimizer import Optimizer
    from asr_amd.superresolution_scripts.superresolution import Superresolution
    opt = Optimizer("adam", 1e-3, amsgrad=True, lr_scheduler=True, decay_steps=60, decay_rate=0.3)
    return Superresolution(1.0, 0.3, 0.7, 0.0, num_iter=iters, num_aug=n, optimizer=opt, feature_size=feat, output_size=out, **kw)


def _labels(small, mode, sr_kw=None, **kw):
    from asr_amd.pipeline import HotPath
    P = _upper()[0]
    model, img, gt, angles, shifts = small
    sr = _sr(**(sr_kw or {}))
    sr.optimizer.optimizer.iterations = 123
    starts = {c: 7 * j + 2 for j, c in enumerate(P.REQ)}
    path = HotPath(model, sr, mode=mode, th_factor=P.TH, batch_size=4)
    return path.run_image_labels(img, angles, shifts, P.REQ, gt_dev=gt, adam_starts=starts, **kw), starts, path


def _confidence(small, kind):
    """The copies' confidence stack [N, fh, fw], made by hand in the path's own forward batches of 4."""
    from asr_amd import ops
    from asr_amd.superresolution_scripts import augmentation_utils as au
    model, img, _, angles, shifts = small
    rows = []
    for i in range(0, len(angles), 4):
        copies = au.augment_on_device(img, angles[i:i + 4], shifts[i:i + 4]).contiguous()
        logits = model.predict_device(copies, batch_size=copies.shape[0])
        rows.append(ops.opm_confidence(logits.contiguous(), kind))
    return torch.cat(rows).contiguous()


def _same(res, ref, keys=("standard",) + SR_KEYS):
    assert sorted(res) == sorted(ref) and res["solved_ids"] == ref["solved_ids"]
    for key in keys:
        assert torch.equal(res[key], ref[key]), key
        assert np.array_equal(res["counts"][key], ref["counts"][key]), key


@pytest.mark.parametrize("mode", ["argmax", "slice_max"])
def test_l2_and_no_weights_is_the_run_without_the_keywords(small, mode):
    P = _upper()[0]
    from asr_amd.pipeline import HotPath
    model, img, gt, angles, shifts = small
    # the solver of the existing tests, built without any of the new keywords
    old = P._sr("adam", 6, 5, (16, 16), (64, 64), False)
    old.optimizer.optimizer.iterations = 123
    starts = {c: 7 * j + 2 for j, c in enumerate(P.REQ)}
    plain = HotPath(model, old, mode=mode, th_factor=P.TH, batch_size=4).run_image_labels(
        img, angles, shifts, P.REQ, gt_dev=gt, adam_starts=starts, keep_scores=True)
    for sr_kw, kw in (({}, {"df_weights": None}), ({"df_loss": "l2", "df_delta": 0.3}, {}), ({"df_loss": None}, {"df_weights": None})):
        res = _labels(small, mode, sr_kw, keep_scores=True, **kw)[0]
        _same(res, plain)
        for t in SR_KEYS:
            for a, r in zip(res["scores"][t], plain["scores"][t]):
                assert (a is None and r is None) or torch.equal(a, r), t
    # without "aug" the option launches nothing and changes nothing
    a = _labels(small, mode, sr_types=("max", "mean"))[0]
    b = _labels(small, mode, {"df_loss": "huber"}, sr_types=("max", "mean"), df_weights="margin")[0]
    _same(b, a, ("standard", "max", "mean"))
    # Huber reaches the class solve and, in slice_max, the max maps' solve; max / mean never see it
    hub = _labels(small, mode, {"df_loss": "huber", "df_delta": 0.05}, keep_scores=True)[0]
    assert not torch.equal(hub["scores"]["aug"][0], plain["scores"]["aug"][0])
    if mode == "slice_max":
        assert not torch.equal(hub["scores"]["aug"][1], plain["scores"]["aug"][1])
    for t in ("max", "mean"):
        assert torch.equal(hub[t], plain[t]) and torch.equal(hub["scores"][t][0], plain["scores"][t][0])
    assert torch.equal(hub["standard"], plain["standard"])


@pytest.mark.parametrize("kind", ["maxprob", "margin"])
def test_confidence_weights_are_the_manual_confidence_and_class_solve(small, kind):
    from asr_amd import ops
    P = _upper()[0]
    _, img, gt, angles, shifts = small
    sr_kw = {"df_loss": "huber", "df_delta": 0.1} if kind == "maxprob" else {}
    res, starts, path = _labels(small, "argmax", sr_kw, keep_scores=True, df_weights=kind, coverages=[50, 100], keep_uncertainty=True)
    solved, stacks = res["solved_ids"], res["uncertainty_stacks"]
    assert len(solved) >= 2 and stacks.shape[0] == len(solved)
    conf = _confidence(small, kind)
    assert conf.shape == stacks.shape[1:] and float(conf.min()) >= 0.0 and float(conf.max()) <= 1.0 and float(conf.std()) > 0
    fshifts = path._sr_frame(img, shifts)
    sr = _sr(**sr_kw)
    scores = sr.augmented_superresolution_classes(stacks, angles, fshifts, [starts[c] for c in solved], df_weights=conf)[0]
    assert torch.equal(scores, res["scores"]["aug"][0])
    labels, counts = ops.fuse_labels(scores, solved, th_factor=P.TH, truth=gt, classes=21)
    assert torch.equal(labels, res["aug"]) and np.array_equal(res["counts"]["aug"], counts.cpu().numpy())
    assert path.sr.optimizer.optimizer.iterations == 123
    # the weights matter, and only to the solve
    plain = _labels(small, "argmax", sr_kw, keep_scores=True)[0]
    assert not torch.equal(plain["scores"]["aug"][0], scores)
    for t in ("max", "mean"):
        assert torch.equal(res[t], plain[t])
    # slice_max: the same stack weights the max maps' solve
    res2, starts2, _ = _labels(small, "slice_max", sr_kw, keep_scores=True, df_weights=kind)
    plain2 = _labels(small, "slice_max", sr_kw, keep_scores=True)[0]
    assert not torch.equal(res2["scores"]["aug"][0], plain2["scores"]["aug"][0])
    assert not torch.equal(res2["scores"]["aug"][1], plain2["scores"]["aug"][1])


def test_superresolution_solves_reach_the_data_term(dev):
    """augmented_superresolution / _batch / _classes and loss_function under df_loss and df_weights against ops.sr_solve and
    ops.sr_loss_terms with the same data term; copy_dropout masks the weights with the copies."""
    from asr_amd import ops
    from test_gpu_warp_sr import _sr_problem
    H, h, n, iters = 64, 16, 6, 4
    y, angs, shs = _sr_problem(61, 2, n, H, h)
    yd = ops.to_device(y)
    g = torch.Generator(dev).manual_seed(3)
    w_shared = torch.rand((n, h, h), device=dev, generator=g)
    w_batch = torch.rand((2, n, h, h), device=dev, generator=g)
    kw = dict(n=n, iters=iters, feat=(h, h), out=(H, H))
    for sr_kw, dt in (({"df_loss": "huber", "df_delta": 0.05}, ("huber", 0.05)), ({"df_loss": "l1"}, "l1"), ({}, None)):
        for wts in (None, w_shared, w_batch):
            if dt is None and wts is None:
                continue
            sr = _sr(**kw, **sr_kw)
            got, terms = sr.augmented_superresolution_batch(yd, angs, shs, df_weights=wts)
            ref_sr = _sr(**kw)
            alphas = np.stack([ref_sr.optimizer.schedule_alphas(iters) for _ in range(2)], axis=1)
            rot, tr = ref_sr._transforms(angs, shs, dev)
            irot, itr = ref_sr._transforms(angs, shs, dev, inverse=True)
            state = ref_sr.optimizer.optimizer
            want, t_want = ops.sr_solve(ops.sr_init_target(yd, (H, H)), yd, rot, tr, irot, itr, ops.to_device(alphas), ref_sr._lambdas,
                                        cfg=state.config(use_btv=False), slot_init=state.slot_init, data_term=dt, weights=wts)
            assert torch.equal(got, want), (dt, None if wts is None else tuple(wts.shape))
            np.testing.assert_allclose(terms.cpu().numpy(), t_want.cpu().numpy(), rtol=1e-12)
            plain, _ = _sr(**kw).augmented_superresolution_batch(yd, angs, shs)
            assert not torch.equal(got, plain)
            # the single-image surface and the classes' surface are the batch's
            if wts is None or wts.dim() == 3:
                one, loss = _sr(**kw, **sr_kw).augmented_superresolution(y[0][..., None], angs[0], shs[0], df_weights=wts)
                assert np.array_equal(one[..., 0], got[0].cpu().numpy()) and np.isfinite(loss)
                cls = _sr(**kw, **sr_kw).augmented_superresolution_classes(yd[:1].repeat(3, 1, 1, 1), angs[0], shs[0], [0, 0, 0],
                                                                         df_weights=wts)[0]
                for k in range(3):
                    assert torch.equal(cls[k], got[0])
                # loss_function: the data term's sum on the raw residual
                x0 = got[0].cpu().numpy()
                lf = _sr(**kw, **sr_kw).loss_function(x0, y[0][..., None], angs[0], shs[0], df_weights=wts)
                _, r = ops.sr_forward_residual(got[:1].contiguous(), yd[:1].contiguous(), rot[:1].contiguous(), tr[:1].contiguous(),
                                               data_term=dt, weights=wts, want_raw=True)
                t = ops.sr_loss_terms(got[:1].contiguous(), r, data_term=dt, weights=wts).cpu().numpy()[0]
                assert lf == pytest.approx(_sr(**kw)._loss_from_terms(t), rel=1e-6)
    # copy_dropout: the frozen mask drops the weights' copies with the stacks'
    drop = _sr(**kw, df_loss="huber", copy_dropout=0.34)
    np.random.seed(5)
    got, _ = drop.augmented_superresolution_batch(yd, angs, shs, df_weights=w_batch)
    mask = drop._drop_mask(int(n * 0.34))
    assert mask.sum() == n - 2
    keep = torch.as_tensor(mask, device=dev)
    full = _sr(n=n, iters=iters, feat=(h, h), out=(H, H), df_loss="huber")
    x0 = ops.sr_init_target(yd, (H, H))                                      # from copy 0 of the FULL stack
    rot, tr = full._transforms(angs[:, mask], shs[:, mask], dev)
    irot, itr = full._transforms(angs[:, mask], shs[:, mask], dev, inverse=True)
    alphas = np.stack([full.optimizer.schedule_alphas(iters) for _ in range(2)], axis=1)
    state = full.optimizer.optimizer
    want, _ = ops.sr_solve(x0, yd[:, keep].contiguous(), rot, tr, irot, itr, ops.to_device(alphas), full._lambdas,
                           cfg=state.config(use_btv=False), slot_init=state.slot_init, data_term=("huber", 0.1),
                           weights=w_batch[:, keep].contiguous())
    assert torch.equal(got, want)


def test_verbose_print_outs_keep_working(dev, capsys):
    from asr_amd import ops
    from test_gpu_warp_sr import _sr_problem
    H, h, n = 64, 16, 4
    y, angs, shs = _sr_problem(63, 1, n, H, h)
    w = torch.rand((n, h, h), device=dev, generator=torch.Generator(dev).manual_seed(4))
    quiet, _ = _sr(n=n, iters=12, feat=(h, h), out=(H, H), df_loss="huber").augmented_superresolution_batch(
        ops.to_device(y), angs, shs, df_weights=w)
    loud, _ = _sr(n=n, iters=12, feat=(h, h), out=(H, H), df_loss="huber", verbose=True).augmented_superresolution_batch(
        ops.to_device(y), angs, shs, df_weights=w)
    assert torch.equal(loud, quiet)
    lines = [l for l in capsys.readouterr().out.splitlines() if "-- loss =" in l]
    assert [l.split()[0] for l in lines] == ["1/12", "11/12", "12/12"]


def test_compute_SR_with_a_data_term(dev, tmp_path):
    from asr_amd.superresolution_scripts.superres_utils import compute_SR, threshold_image
    from test_gpu_realign_covered import _golden, _sr as _sr_golden
    _path, n, lr, hr, masks, max_masks, angles, shifts, name = _golden("slice_max")
    wts = torch.rand((n,) + tuple(lr), device=dev, generator=torch.Generator(dev).manual_seed(6))
    fresh = lambda **kw: _sr_golden(lr, hr, n, **kw)                       # a fresh Adam counter for every solve
    got = compute_SR(fresh(df_loss="huber", df_delta=0.2), masks, angles, shifts, name, str(tmp_path), SR_type="aug",
                     max_masks=max_masks, class_id=8, df_weights=wts)
    sr = fresh(df_loss="huber", df_delta=0.2)
    target = sr.augmented_superresolution(masks, angles, shifts, df_weights=wts)[0]
    t_max = sr.augmented_superresolution(max_masks, angles, shifts, df_weights=wts)[0]
    assert np.array_equal(got, threshold_image(target, 8, th_mask=t_max))
    assert not np.array_equal(fresh().augmented_superresolution(masks, angles, shifts)[0], target)
    assert not np.array_equal(fresh(df_loss="huber", df_delta=0.2).augmented_superresolution(masks, angles, shifts)[0], target)
    with pytest.raises(ValueError, match="'aug'"):
        compute_SR(fresh(), masks, angles, shifts, name, str(tmp_path), SR_type="mean", df_weights=wts)


def test_bad_options_raise_before_the_model_runs(small):
    from asr_amd.pipeline import HotPath
    P = _upper()[0]
    model, img, gt, angles, shifts = small
    sr = _sr()
    path = HotPath(model, sr, mode="argmax", th_factor=P.TH, batch_size=4)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats().get("allocation.all.allocated", 0)
    for bad in ("entropy", 0.5, ("maxprob",), True):
        with pytest.raises(ValueError, match="df_weights must be None or one of"):
            path.run_image_labels(img, angles, shifts, P.REQ, gt_dev=gt, df_weights=bad)
    for bad in (dict(df_loss="l3"), dict(df_loss="huber", df_delta=-0.1), dict(df_loss="huber", df_delta=float("inf"))):
        with pytest.raises(ValueError, match="df_loss"):
            _sr(**bad)
    with pytest.raises(ValueError, match="df_weights must be"):
        sr.augmented_superresolution_batch(None, angles[None], shifts[None], df_weights=np.ones((6, 16, 16), np.float32))
    assert torch.cuda.memory_stats().get("allocation.all.allocated", 0) == before      # not one device allocation
    assert sr.optimizer.optimizer.iterations == 0


@pytest.mark.parametrize("activation", ["softmax", "sigmoid"])
def test_confidence_is_taken_from_logits_whatever_the_model_returns(small, activation):
    """A model with a last_activation returns probabilities; the argmax OPM of those is the logits', so with the confidence
    made from the batch's raw logits every result is the un-activated model's bit for bit (a second softmax over the
    probabilities would give other weights)."""
    model = small[0]
    want = _labels(small, "argmax", {"df_loss": "huber"}, keep_scores=True, df_weights="maxprob")[0]
    assert model.last_activation is None
    model.last_activation = activation
    try:
        got = _labels(small, "argmax", {"df_loss": "huber"}, keep_scores=True, df_weights="maxprob")[0]
    finally:
        model.last_activation = None
    _same(got, want)
    assert torch.equal(got["scores"]["aug"][0], want["scores"]["aug"][0])


def test_df_loss_reaches_every_solve_of_the_path(small, monkeypatch, tmp_path):
    """HotPath and the evaluations solve through their Superresolution object: under df_loss="huber" every ops.sr_solve they
    make carries the data term (and, with df_weights, the confidence stack); under the default none does."""
    from PIL import Image
    from bench import synth_image
    from asr_amd import ops
    from asr_amd.evaluation import evaluate_labelmaps, evaluate_precomputed
    from asr_amd.pipeline import HotPath
    from test_gpu_realign_covered import _golden, _sr as _sr_golden
    P = _upper()[0]
    model, img, gt, angles, shifts = small
    seen = []
    real = ops.sr_solve

    def recording(*a, **kw):
        seen.append((kw.get("data_term"), kw.get("weights")))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "sr_solve", recording)
    hub = {"df_loss": "huber", "df_delta": 0.05}

    def runs(sr_kw):
        del seen[:]
        out = [HotPath(model, _sr(**sr_kw), class_id=8, mode="argmax", th_factor=P.TH, batch_size=4).run_image(
            img, angles, shifts, gt_dev=gt)["aug"]]
        res = HotPath(model, _sr(**sr_kw), mode="slice_max", th_factor=P.TH, batch_size=4).run_image_classes(
            img, angles, shifts, [3, 8], gt_dev=gt)
        out += [res[3]["aug"], res[8]["aug"]]
        return out, list(seen)

    plain, calls = runs({})
    assert len(calls) == 3 and all(c == (None, None) for c in calls), calls          # run_image, classes and their max maps
    robust, calls = runs(hub)
    assert len(calls) == 3 and all(c == (("huber", 0.05), None) for c in calls), calls
    assert all(a.shape == b.shape for a, b in zip(plain, robust))
    # evaluate_labelmaps, with the confidence weights
    images, gts = [], []
    arr = synth_image(np.random.default_rng(21), 64)
    images.append(str(tmp_path / "0.png"))
    Image.fromarray(np.clip(np.rint(arr * 255.0), 0, 255).astype(np.uint8), mode="RGB").save(images[-1])
    gts.append(str(tmp_path / "gt0.png"))
    Image.fromarray(gt.cpu().numpy().astype(np.uint8), mode="L").save(gts[-1])
    run = lambda sr_kw, **kw: evaluate_labelmaps(HotPath(model, _sr(**sr_kw), mode="argmax", th_factor=P.TH, batch_size=4), images, gts,
                                                 P.REQ, num_aug=6, angle_max=0.15, shift_max=8, img_size=(64, 64), **kw)
    del seen[:]
    ref = run({})
    assert seen and all(c == (None, None) for c in seen)
    del seen[:]
    out = run(hub, df_weights="margin")
    assert seen and all(c[0] == ("huber", 0.05) and tuple(c[1].shape) == (6, 16, 16) for c in seen), seen
    assert out.rows.shape == ref.rows.shape and out.counts.shape == ref.counts.shape
    for j in (0, 2, 3):                                                     # standard, max, mean: the solver options are not theirs
        assert np.array_equal(out.counts[j], ref.counts[j])
    # evaluate_precomputed
    path, n, lr, hr, masks, max_masks, a, s, name = _golden("argmax")
    g = np.zeros(hr, np.uint8)
    g[hr[0] // 4:3 * hr[0] // 4, hr[1] // 4:3 * hr[1] // 4] = 8
    (tmp_path / "gt").mkdir()
    Image.fromarray(g, mode="L").save(tmp_path / "gt" / f"{name}.png")
    kw = dict(num_aug=n, class_id=8, th_factor=0.3, img_size=hr, out_dir=str(tmp_path / "out"))
    del seen[:]
    evaluate_precomputed(_sr_golden(lr, hr, n), [path], str(tmp_path / "gt"), **kw)
    assert seen == [(None, None)]
    del seen[:]
    evaluate_precomputed(_sr_golden(lr, hr, n, df_loss="l1"), [path], str(tmp_path / "gt"), **kw)
    assert seen == [(("l1", None), None)] or seen == [(("l1", 0.1), None)], seen
