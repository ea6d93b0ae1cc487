"""The whole hot path for one image, device-resident end to end:

    augment (N copies) -> DeepLabV3+ forward -> OPM -> {ASR solve, max-SR, mean-SR} -> threshold
    -> IoU counts

i.e. the body of test_SR.py:73-94 / generate_augmented_copies.py:88-91 + SR_single_class.py:83-127
without the host round trips (ndarray lists, HDF5) the reference puts between the stages.
Used by bench.py, the scripts and the smoke test.
"""
from __future__ import annotations

import contextlib
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .label_record import counts_name, label_fields, label_layout
from .superresolution_scripts import augmentation_utils as au
from .utils import (coverage_edges, coverage_retained, iou_from_counts, mean_iou_from_counts, opm_scales,
                    uncertainty_map)


class HotPath:
    def __init__(self, model, superresolution, class_id=8, mode="argmax", th_factor=0.15, batch_size=16):
        self.model = model
        self.sr = superresolution
        self.class_id = class_id
        self.mode = mode
        self.th_factor = th_factor
        self.batch_size = batch_size
        self._side = None
        self._lanes = {}

    def _threshold(self, target, target_max, out=None):
        if target_max is not None:
            return ops.threshold(target, self.class_id, th_mask=target_max, out=out)
        return ops.threshold(target, self.class_id, th_factor=self.th_factor, out=out)

    MASK_KEYS = ("standard", "aug", "max", "mean")          # rows of the per-image mask buffer

    def standard_mask(self, logits0, out_hw, out=None):
        """generate_standard_output.py:52-65: final bilinear upsample + argmax + class filter, from the
        logits of the un-augmented copy 0 (one kernel)."""
        return ops.standard_mask(logits0.contiguous(), out_hw, self.class_id, out=out)

    # ---- stage 1 (model stream): augment -> forward -> OPM (-> standard output) ------------------------
    def _forward_stacks(self, image_dev, angles, shifts, planes, opm, logits0=None, profile=None, lane=0, confidence=None):
        """The copies go through the model one forward batch at a time (augmentation_utils.py:30-59 draws them in chunks
        for the same reason): each batch is augmented straight into the plan's input buffer, its logits are consumed in
        place by the OPM, which writes its rows of the image's stacks -- nothing of size [N,H,W,3] or [N,h,w,classes]
        outlives a batch.  planes: 1, or the K classes of a class set.  opm(preds, out_rows, out_max_rows) fills the batch's
        rows [planes, k, fh, fw] of the stacks (out_max_rows: None unless slice_max); logits0, when given, gets copy 0's
        logits [fh, fw, C] (the standard output is made from them).  confidence(preds, first, k, n), when given, is called
        next to the OPM with each batch's logits [k, fh, fw, C], the copies first .. first + k - 1 of n (run_image_labels
        fills its per-copy confidence stack there).  Returns the raw stacks y, ymax [planes, N, fh, fw]."""
        n = len(angles)
        h, w, _ = image_dev.shape
        eng = self.model.engine
        bs = min(self.batch_size, n)
        y = ymax = None                     # allocated from the first batch's logits: their size depends on the
        for i in range(0, n, bs):
            k = min(bs, n - i)
            copies = au.augment_on_device(image_dev, angles[i:i + k], shifts[i:i + k], out=eng.input_view(k, h, w, lane))
            preds = self.model.predict_device(copies, batch_size=k, profile=profile, lane=lane, clone=False)  # logits stay there
            if y is None:                   # decoder / upsampling options, not only on the backbone's stride
                y = torch.empty((planes, n) + tuple(preds.shape[1:3]), dtype=torch.float32, device=image_dev.device)
                ymax = torch.empty_like(y) if self.mode == "slice_max" else None
            if i == 0 and logits0 is not None:
                logits0(self.model.logits_of(preds, 0).contiguous())
            opm(preds, y[:, i:i + k], ymax[:, i:i + k] if ymax is not None else None)
            if confidence is not None:
                confidence(preds, i, k, n)
            del copies, preds
        return y, ymax

    def _stage_model(self, image_dev, angles, shifts, profile=None, want_standard=True, lane=0):
        """Stage 1 of the single class: (res with the mask buffer and the standard mask, normalised y, ymax [1, N, fh, fw])."""
        out_hw = self.sr.output_size
        res = {"_masks": torch.empty((len(self.MASK_KEYS),) + tuple(out_hw), dtype=torch.int32, device=image_dev.device)}
        opm = lambda preds, out, out_max: au.output_processing(preds, self.class_id, self.mode, out=out[0],
                                                               out_max=out_max[0] if out_max is not None else None)

        def standard(logits0):
            res["standard"] = self.standard_mask(logits0, out_hw, out=res["_masks"][0])

        y, ymax = self._forward_stacks(image_dev, angles, shifts, 1, opm, standard if want_standard else None, profile, lane)
        return (res,) + self._normalise(y, ymax)

    def _classes_stage_model(self, image_dev, angles, shifts, ids, profile, standard, confidence=None):
        """Stage 1 of a class set: the OPM of every class into raw [K, N, h, w] stacks (y, ymax).
        standard: None, or a function of copy 0's logits [h, w, C] (the standard masks / label map are made from them)."""
        opm = lambda preds, out, out_max: au.output_processing_classes(preds, ids, self.mode, out=out, out_max=out_max)
        return self._forward_stacks(image_dev, angles, shifts, len(ids), opm, standard, profile, confidence=confidence)

    def _normalise(self, y, ymax):
        """load_SR_data's global min-max normalisation of each plane's stack to [0, 1] (superres_utils.py:183-206); not in
        slice mode."""
        if self.mode != "slice":
            y = ops.minmax_normalize(y, segments=y.shape[0], new_min=0.0, new_max=1.0)
            if ymax is not None:
                ymax = ops.minmax_normalize(ymax, segments=ymax.shape[0], new_min=0.0, new_max=1.0)
        return y, ymax

    def _sr_frame(self, image_dev, shifts):
        """The SR stage applies the copies' shifts in ITS pixel frame (superresolution.py:61-64 translates the HR estimate,
        of output_size).  The reference always runs with image size == output_size; when they differ (BASELINE configs[4]:
        1024 x 1024 inputs, 512 x 512 SR output) a shift of s input pixels is s * output_size / image_size output pixels
        (per axis; shifts are [dx, dy]).  Angles are frame-independent."""
        h, w, _ = image_dev.shape
        H, Wd = self.sr.output_size
        if (h, w) == (H, Wd):
            return shifts
        return (np.asarray(shifts, dtype=np.float32) * np.array([Wd / w, H / h], dtype=np.float32)).astype(np.float32)

    # ---- stage 2 (any stream): ASR solve, max / mean realign, threshold, IoU counts --------------------
    def _sr_scores(self, y, ymax, angles, fshifts, sr_types, solve):
        """Stage 2 up to the SR outputs: yields (t, scores [P, H, W], max-map scores [P, H, W] | None) for each SR type, the P
        planes of the stacks as a batch of the solver / realign.  solve(stack, a, s, second) -> [P, H, W] is the ASR solve of a
        stack under the angles a [P, N] and shifts s [P, N, 2]; second: the stack is the max map, solved after y."""
        sr = self.sr
        a = np.repeat(np.asarray(angles, dtype=np.float32)[None], y.shape[0], axis=0)
        s = np.repeat(np.asarray(fshifts, dtype=np.float32)[None], y.shape[0], axis=0)
        both = None
        if "max" in sr_types and "mean" in sr_types:            # one pass over the copies serves both (bit-identical)
            both = (sr.realign_batch(y, a, s, "both"), sr.realign_batch(ymax, a, s, "both") if ymax is not None else None)
        for t in sr_types:
            if t == "aug":
                tgt = solve(y, a, s, False)
                tmax = solve(ymax, a, s, True) if ymax is not None else None
            elif both is not None:
                j = 0 if t == "max" else 1
                tgt, tmax = both[0][j], (both[1][j] if both[1] is not None else None)
            else:
                tgt = sr.realign_batch(y, a, s, t)
                tmax = sr.realign_batch(ymax, a, s, t) if ymax is not None else None
            yield t, tgt, tmax

    def _stage_sr(self, res, y, ymax, angles, shifts, gt_dev, adam_start, sr_types):
        sr = self.sr

        def solve(stack, a, s, second):     # the max map's solve goes on from where y's left the Adam counter
            if adam_start is not None and not second:
                sr.optimizer.optimizer.iterations = adam_start
            return sr.augmented_superresolution_batch(stack, a, s)[0]

        for t, tgt, tmax in self._sr_scores(y, ymax, angles, shifts, sr_types, solve):
            res[t] = self._threshold(tgt[0], tmax[0] if tmax is not None else None,
                                     out=res["_masks"][self.MASK_KEYS.index(t)])
        if gt_dev is not None:
            res["_iou_keys"], res["_iou_counts"] = self._iou_counts(res, gt_dev)
        return res

    @staticmethod
    @contextlib.contextmanager
    def _sr_stage_timed(profile):
        """What runs inside (the SR stage: solve, realign, thresholds or fusion, counts) as one HIP-event interval, added to
        profile["_sr_stage_ms"]; nothing with profile None."""
        if profile is None:
            yield
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        yield
        e1.record()
        torch.cuda.synchronize()
        profile["_sr_stage_ms"] = profile.get("_sr_stage_ms", 0.0) + e0.elapsed_time(e1)

    def run_image(self, image_dev, angles, shifts, gt_dev=None, adam_start=None, profile=None,
                  sr_types=("aug", "max", "mean"), want_standard=True):
        """image_dev [H,W,3] float32 device; angles [N], shifts [N,2] float32 host arrays;
        gt_dev [H,W] int32 device labels (optional).  Returns dict of device masks (+ 6 IoUs)."""
        res, y, ymax = self._stage_model(image_dev, angles, shifts, profile, want_standard)
        with self._sr_stage_timed(profile):
            res = self._stage_sr(res, y, ymax, angles, self._sr_frame(image_dev, shifts), gt_dev, adam_start, sr_types)
        return self._finish(res)

    def submit_image(self, image_dev, angles, shifts, gt_dev=None, adam_start=None,
                     sr_types=("aug", "max", "mean"), want_standard=True):
        """Pipelined form: stage 1 on the current stream, stage 2 on a side HIP stream, so the latency-bound
        SR solve of image i runs under the MFMA-bound forward pass of image i+1.  Returns a handle whose
        .result() waits for the side stream and yields the same dict as run_image."""
        main = torch.cuda.current_stream()
        if self._side is None:
            # high priority: the SR stage is a chain of short launches that must slip in between the forward pass's
            # workgroups as they retire, not queue behind a whole GEMM grid
            self._side = torch.cuda.Stream(priority=-1)
        res, y, ymax = self._stage_model(image_dev, angles, shifts, None, want_standard)
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(self._side):
            self._side.wait_event(ready)
            res = self._stage_sr(res, y, ymax, angles, self._sr_frame(image_dev, shifts), gt_dev, adam_start, sr_types)
            done = torch.cuda.Event()
            done.record(self._side)
        for t in [y, ymax] + [v for v in res.values() if isinstance(v, torch.Tensor)]:
            if t is not None:
                t.record_stream(self._side)          # allocated on the main stream, consumed on the side stream
        return _Pending(self, res, done, keep=(y, ymax, gt_dev))

    def submit_lane(self, lane, image_dev, angles, shifts, gt_dev=None, adam_start=None,
                    sr_types=("aug", "max", "mean"), want_standard=True):
        """Two-lane pipelining: the WHOLE image (both stages) runs on the HIP stream of `lane`, with that lane's own
        activation pool, so consecutive images submitted to alternating lanes overlap like two independent processes
        (the forward pass of one under the SR solve, realign and reductions of the other, and vice versa).  Results
        are bit-identical to run_image; .result() of the returned handle waits for the lane."""
        if lane not in self._lanes:
            self._lanes[lane] = torch.cuda.Stream()
        stream = self._lanes[lane]
        stream.wait_stream(torch.cuda.current_stream())        # inputs prepared on the caller's stream
        with torch.cuda.stream(stream):
            res, y, ymax = self._stage_model(image_dev, angles, shifts, None, want_standard, lane=lane)
            res = self._stage_sr(res, y, ymax, angles, self._sr_frame(image_dev, shifts), gt_dev, adam_start, sr_types)
            done = torch.cuda.Event()
            done.record(stream)
        return _Pending(self, res, done, keep=(y, ymax, gt_dev, image_dev))

    # ---- class sets: several classes of one image from ONE forward pass --------------------------------------------------
    @property
    def _solves(self):
        """ASR solves per class: its map's, and in slice_max its max map's."""
        return 2 if self.mode == "slice_max" else 1

    def _class_starts(self, ids, adam_starts):
        """Global Adam step counter before each class's solve: adam_starts[c], or consecutive solves in the order of ids
        from the current counter."""
        sr = self.sr
        if adam_starts is None:
            it0 = sr.optimizer.optimizer.iterations if sr.optimizer is not None else 0
            return [it0 + j * self._solves * sr.num_iter for j in range(len(ids))]
        return [int(adam_starts[c]) for c in ids]

    def _classes_scores(self, y, ymax, angles, fshifts, starts, sr_types, tv_weights=None, df_weights=None, stop=None,
                        iters=None, couple=False, reweight=None, copy_weights=None):
        """_sr_scores of a class set: class k's solve starts at the Adam step starts[k], its max map's num_iter later; the
        counter itself is left as it was.  tv_weights: the image's edge weights (wy, wx), shared by every solve; df_weights:
        the copies' confidence stack [N, h, w], the weights of every solve's data term.  stop (a checked monitor dict): the
        solves run under it, and iters (a dict) receives the device int32 [K] iterations of each: "aug", "aug_max".
        couple: the K classes are one coupled solve (Superresolution.augmented_superresolution_classes' couple).
        reweight (a checked reweight dict): the solves reweight their copies under it, and copy_weights (a dict) receives the
        device float32 [K, N] weights of each: "aug", "aug_max"."""
        sr = self.sr
        kw = {} if tv_weights is None else {"tv_guide": tv_weights}
        if df_weights is not None:
            kw["df_weights"] = df_weights
        if couple:
            kw["couple"] = True
        solve = lambda stack, a, s, second: sr.augmented_superresolution_classes(
            stack, a[0], s[0], [st + second * sr.num_iter for st in starts], **kw)[0]
        if stop is not None:
            plain = solve

            def solve(stack, a, s, second):
                saved, sr.monitor, sr.last_trace = sr.monitor, stop, None
                try:
                    x = plain(stack, a, s, second)
                finally:
                    sr.monitor = saved
                if sr.last_trace is not None:              # (num_iter = 0: no solve, no trace)
                    iters["aug_max" if second else "aug"] = sr.last_trace.iters_done
                return x
        if reweight is not None:
            inner = solve

            def solve(stack, a, s, second):
                saved, sr.reweight, sr.last_copy_weights = sr.reweight, reweight, None
                try:
                    x = inner(stack, a, s, second)
                finally:
                    sr.reweight = saved
                if sr.last_copy_weights is not None:       # (num_iter = 0: no solve, no weights)
                    copy_weights["aug_max" if second else "aug"] = sr.last_copy_weights.weights
                return x
        return self._sr_scores(y, ymax, angles, fshifts, sr_types, solve)

    @staticmethod
    def check_sr_reweight(sr_reweight):
        """run_image_labels' sr_reweight, checked on the host before any launch: None, a kind name ("cauchy", "hard") or a dict
        with any of kind, kappa (default 2), every (10), start (10) -> None or the reweight dict of the solver (no history)."""
        if sr_reweight is None:
            return None
        if isinstance(sr_reweight, str):
            sr_reweight = dict(kind=sr_reweight)
        if not isinstance(sr_reweight, dict) or set(sr_reweight) - {"kind", "kappa", "every", "start"}:
            raise ValueError(f"sr_reweight must be a kind name or a dict with keys among kind, kappa, every, start, got {sr_reweight!r}")
        return ops.check_sr_reweight(dict(sr_reweight, history=False), "sr_reweight")

    @staticmethod
    def check_sr_stop(sr_stop):
        """run_image_labels' sr_stop, checked on the host before any launch: None, or a dict with any of rel_tol (default
        1e-4), patience (3), every (1), min_iter (0) -> None or the monitor dict of the solver (no history is kept)."""
        if sr_stop is None:
            return None
        if not isinstance(sr_stop, dict) or set(sr_stop) - {"rel_tol", "patience", "every", "min_iter"}:
            raise ValueError(f"sr_stop must be a dict with keys among rel_tol, patience, every, min_iter, got {sr_stop!r}")
        return ops.check_sr_monitor(dict(sr_stop, history=False), "sr_stop")

    def _advance_past(self, starts, adam_starts, sr_types):
        """adam_starts None: the classes counted as consecutive solves, the counter moves past the last of them."""
        if adam_starts is None and "aug" in sr_types and self.sr.optimizer is not None and starts:
            self.sr.optimizer.optimizer.iterations = starts[-1] + self._solves * self.sr.num_iter

    @staticmethod
    def _gt_int32(gt_dev):
        """The ground truth as a contiguous int32 device tensor."""
        return (gt_dev if gt_dev.dtype == torch.int32 else gt_dev.to(torch.int32)).contiguous()

    def run_image_classes(self, image_dev, angles, shifts, class_ids, gt_dev=None, adam_starts=None,
                          sr_types=("aug", "max", "mean"), want_standard=True, profile=None):
        """run_image for every class of `class_ids` (K distinct ids, K <= 32) with one pass of the N copies through the model.
        Returns {class_id: dict}, each dict equal bit for bit to HotPath(model, sr, class_id=c, mode, th_factor,
        batch_size).run_image(image_dev, angles, shifts, gt_dev, adam_start=adam_starts[c], sr_types=sr_types,
        want_standard=want_standard) -- the classes keep the reference's single-class meaning; run_image_labels fuses them.

        adam_starts: {class_id: global Adam step counter before that class's solve} (a slice_max class's max-map solve
        starts num_iter later, as run_image's second solve does); the counter is left as it was.  None: the classes count
        as consecutive run_image calls in the order of class_ids, from the current counter, which advances past them."""
        ids = [int(c) for c in class_ids]
        starts = self._class_starts(ids, adam_starts)
        out_hw = self.sr.output_size
        masks = torch.empty((len(self.MASK_KEYS), len(ids)) + tuple(out_hw), dtype=torch.int32, device=image_dev.device)
        have = []

        def standard(logits0):
            ops.standard_mask_classes(logits0, out_hw, ids, out=masks[0])
            have.append("standard")

        y, ymax = self._classes_stage_model(image_dev, angles, shifts, ids, profile, standard if want_standard else None)
        y, ymax = self._normalise(y, ymax)
        # stage 2: the K classes as a batch of the existing solver / realign, then K-class threshold and IoU counts
        with self._sr_stage_timed(profile):
            for t, tgt, tmax in self._classes_scores(y, ymax, angles, self._sr_frame(image_dev, shifts), starts, sr_types):
                row = masks[self.MASK_KEYS.index(t)]
                if tmax is not None:
                    ops.threshold_classes(tgt, ids, th_mask=tmax, out=row)
                else:
                    ops.threshold_classes(tgt, ids, th_factor=self.th_factor, out=row)
                have.append(t)
            self._advance_past(starts, adam_starts, sr_types)
            keys = [key for key in self.MASK_KEYS if key in have]
            counts = None
            if gt_dev is not None:
                preds = masks[[self.MASK_KEYS.index(key) for key in keys]].transpose(0, 1).contiguous()     # [K, M, H, W]
                counts = ops.iou_counts_classes(self._gt_int32(gt_dev), preds, ids, include_bg=True)
        counts = counts.cpu().numpy() if counts is not None else None
        out = {}
        for j, c in enumerate(ids):
            res = {key: masks[self.MASK_KEYS.index(key), j] for key in keys}
            if counts is not None:
                res["ious"] = self._ious_from_counts(keys, counts[j])
            out[c] = res
        return out

    # ---- label maps: the classes of an image fused into one label map per SR type, and its Mean_IOU -----------------------
    def run_image_labels(self, image_dev, angles, shifts, class_ids=range(1, 21), gt_dev=None, adam_starts=None,
                         sr_types=("aug", "max", "mean"), want_standard=True, prune=True, profile=None, keep_scores=False,
                         band_widths=None, band_ignore_label=255, confusion_labels=None, th_factors=None, guide=None,
                         coverages=None, keep_uncertainty=False, min_region=None, df_weights=None, sr_stop=None, couple=False,
                         sr_reweight=None,
                         tv_guide=None, crf=None, segments=None):
        """One label map per SR type from one forward pass: stage 1 and the solves are run_image_classes's; stage 2 ends in the
        fusion kernel (ops.fuse_labels) instead of K thresholds.  class_ids: K <= 32 distinct ids, none 0 (the label of "no
        class").  At each pixel the label is the class whose single-class mask is set there and whose SR output is greatest
        (slice_max: greatest margin over its max map's SR output), the first of class_ids on equal values, 0 where no mask
        is set; the standard label map is the upsampled argmax of copy 0 where it is in class_ids, else 0.

        Returns a dict: "standard" / "aug" / "max" / "mean" -> device int32 [H, W] (those asked for); with gt_dev also
        "counts" {key: int64 [3, 256] numpy, ops.class_counts of the map against gt_dev} and "Mean_IOU" {key: float,
        utils.mean_iou_from_counts}; "solved_ids": the classes that went through the solver; with keep_scores "scores"
        {t: (S [K', H, W], Smax [K', H, W] | None)}, the tensors the fusion read, plane j belonging to solved_ids[j].

        prune (argmax OPM only): a class that wins no pixel of any copy has an all-zero stack; its solve stays at zero
        whatever the update rule or prior (zero data, zero gradient, zero step) and its mask is empty, so it is left out of
        the normalisation, the solver, the realign and the fusion.  The K raw maxima (the min/max kernel that the
        normalisation runs, here ahead of it) are read once on the host to know them: one synchronisation after the
        forward pass.  The label maps, the counts and the Adam bookkeeping are those of
        prune=False bit for bit.  The slice and slice_max stacks are dense: prune does nothing there.
        adam_starts: as run_image_classes; a class's start counts ALL requested ids in order, pruned or not, and with None
        the counter advances past all of them.  Zero classes left is legal: every SR label map is 0.

        band_widths (with gt_dev; 1..16 integers in [1, 64]): the trimap of include/asr_hip.h.  The result gains "band_counts"
        {key: int64 [B, 3, 256] numpy, what utils.trimap_counts gives for that label map} and "band_Mean_IOU" {key: float64
        [B]}, widths in the caller's order; band_ignore_label (-1 or None: none) is left out of every bin.  One distance
        launch on gt_dev, one band-count launch over all label maps, and the same single copy to the host as "counts".
        With band_widths=None nothing else is launched and nothing else returned.

        confusion_labels (with gt_dev; an integer L in [1, 64]): the result gains "confusion" {key: int64 [L+1, L+1] numpy, what
        utils.confusion_matrix(gt, label map, L) gives: truth in the rows, bin L holding void and every other value outside
        0..L-1}.  One launch over all label maps, after the band counts, and the same single copy to the host as "counts".
        With confusion_labels=None nothing else is launched and nothing else returned.

        th_factors (with gt_dev; 1..64 threshold factors, any order; not in slice_max mode, where the threshold plays no part):
        the threshold curve of the label maps.  th_factor is read by the fusion alone, so the SR outputs of this one run hold
        every factor's label map: the result gains "sweep_counts" {t: int64 [T, 3, 256] numpy, row j the "counts" a
        HotPath(th_factor=th_factors[j]) gives for SR type t} and "sweep_Mean_IOU" {t: float64 [T]}, keyed by the SR types asked
        for (the standard map does not depend on the factor).  One sweep call per SR type (ops.fuse_labels_sweep_counts) right
        after its fusion, on the same score tensors, and the same single copy to the host as "counts"; with no class left
        after pruning every factor's counts are the zero map's.  With th_factors=None nothing else is launched and nothing
        else returned.

        guide ((radius, eps); image_dev must be [H, W, 3] at the SR output size): the guided filter of include/asr_hip.h with
        the image itself as the guide moves each score map's boundary onto the image's edges.  The guide-only pass
        (ops.guided_prepare) runs once per image inside the timed SR stage; each SR type's scores (and in slice_max its max
        maps' scores) are refined in place (ops.guided_apply) before the fusion, the sweep counts and keep_scores see them.
        With guide=None nothing else is launched and every result is what it was.

        coverages (with gt_dev; 1..16 whole percentages in [1, 100], any order): the risk-coverage curve of the label maps.
        One ops.realign_moments call over the stacks of the solved classes (the stacks the solver read, frame coverage: one
        shared all-ones plane, valid_min 0.5; in slice_max mode the class planes, not the max maps) gives each class's
        variance over the copies; utils.uncertainty_map takes the maximum over the classes (+inf where a class rests on
        fewer than two copies, and everywhere when no class was solved), utils.coverage_edges picks the p % quantiles among
        the pixels that are not void (255) on the device, and one ops.binned_class_counts call scores every produced label
        map, standard included, over its p % most certain pixels.  The result gains "coverage_counts" {key: int64 [B, 3, 256]
        numpy}, "coverage_Mean_IOU" {key: float64 [B]} and "coverage_share" (float64 [B]: the share of the non-void pixels
        each percentage retained, >= p / 100 as ties stay in), in the same single copy to the host as "counts"; with
        keep_uncertainty also "uncertainty" (device float32 [H, W]) and "uncertainty_stacks" (the [K', N, h, w] tensor the
        moments were taken of, None when no class was solved).  With coverages=None nothing else is launched and nothing
        else returned.

        min_region (an integer A or (A, connectivity), connectivity 4 or 8, default 4; not together with th_factors, whose label
        maps are counted and never written): the clean-up of include/asr_hip.h, "regions".  After the last fusion, inside the
        timed SR stage, one ops.label_regions and one ops.clean_labels call run over all produced label maps at once, the
        standard map included, in place: every region of fewer than A pixels takes the one value of its non-small surround, or
        0.  Everything downstream sees the cleaned maps: the returned maps, "counts" and "Mean_IOU" (recounted with
        ops.class_counts, since the fusion's in-pass counts belong to the raw maps), the trimap, the confusion matrix and the
        risk-coverage counts.  The result gains "regions" {key: int64 [4] numpy: regions, small regions, pixels in small
        regions, pixels changed} and, with gt_dev, "raw_counts" and "raw_Mean_IOU", the scores before the clean-up.  With no
        class left after pruning the zero maps are one region each and the calls still run.  With min_region=None nothing
        else is launched and nothing else returned.

        segments (with gt_dev; an integer L, (L, connectivity) or (L, connectivity, include_zero), ops.check_segments; not together
        with th_factors, whose label maps are counted and never written): the region-by-region score of include/asr_hip.h,
        "segments".  After the last fusion (and after the clean-up when min_region is on), inside the timed SR stage, three calls
        run: one ops.label_regions of the truth, one over all produced label maps, the standard map included, and one
        ops.segment_match.  The result gains "segments" {key: int64 [L, 4] numpy: TP, FP, FN and Q per label, what
        utils.segment_counts gives for that label map; utils.metrics_from_segments} in the same single copy to the host as
        "counts".  With min_region on, the maps before the clean-up are matched too, "raw_segments" {key: int64 [L, 4]}, against
        the same labelling of the truth; the clean-up's labelling of the maps is reused when the two connectivities agree.  With
        segments=None nothing else is launched and nothing else returned.

        tv_guide (beta, a finite number >= 0; image_dev must be [H, W, 3] at the SR output size; not with use_BTV): a solver
        option, not a scoring option -- the image goes INTO the "aug" solves as the edge weights of their TV prior
        (include/asr_hip.h, "edge-weighted TV": w = 1 / (1 + beta * |forward difference of the image|^2)), so a boundary is
        cheap where the image has an edge.  One ops.tv_edge_weights call per image inside the timed SR stage; the pair is
        shared by the K classes' solve and, in slice_max, by the max maps' solve.  Independent of guide (which refines the
        scores afterwards).  beta = 0 gives weights of one: every result is tv_guide=None's bit for bit.  With
        tv_guide=None nothing else is launched and every result is what it was.

        crf (a dict of any of the fields of include/asr_hip.h's asr_crf_config -- radius, dilation, iterations, w_app, w_smooth,
        theta_pos, theta_rgb, theta_smooth; ops.check_crf -- plus tau and standard_conf; image_dev must be [H, W, 3] at the SR
        output size): the windowed CRF of include/asr_hip.h decides each SR type's label map jointly over the classes and the
        image instead of ops.fuse_labels: the map is ops.crf_refine of ops.crf_unaries(scores, th_factor, tau) with the image as
        the guide -- after the guided refinement when guide is on too, inside the timed SR stage -- and its counts are
        ops.class_counts'.  With iterations = 0 and tau <= 1 the map is the fusion's wherever at most one class passes; where
        several pass, the margin over the threshold ranks them, not the score.  standard_conf (default None: the standard map is left alone):
        the standard label map goes through ops.crf_unaries_from_labels(map, class_ids, standard_conf) and ops.crf_refine before
        it is counted.  Everything downstream sees the CRF maps: the clean-up, the segments, the trimap, the confusion matrix
        and the risk-coverage counts.  Refused on the host, before the model: slice_max mode (its pass rule S >= Smax is not a
        threshold, so there is no unary), th_factors (the sweep counts the fusion rule's maps), more than 31 class ids (the CRF has
        at most 32 labels) and an image of another shape.
        With no class left after pruning the SR maps are 0 as before.  With crf=None nothing else is launched and every result is
        what it was.

        df_weights ("maxprob" or "margin"): a solver option -- each low-resolution pixel of each copy enters the "aug" solves'
        data term (include/asr_hip.h, "data term"; the loss itself is the solver's df_loss) with the network's own confidence
        there as its weight: the largest softmax entry of the copy's logits, or the difference of the two largest.  One
        ops.opm_confidence call per forward batch, next to the OPM, fills an [N, fh, fw] stack; it is shared by the K classes'
        solve and, in slice_max, by the max maps' solve, and it is neither pruned nor normalised (copy_dropout drops its
        copies with the stacks').  The kernel always reads logits: from a model with a last_activation the batch's raw logits
        are taken, not the probabilities it returns (with final_upsample as well there are none at the stacks' size: refused).  With df_weights=None, or without "aug" in sr_types, nothing else is launched and every
        result is what it was.

        sr_stop ({"rel_tol": .., "patience": .., "every": .., "min_iter": ..}, any subset; check_sr_stop): the "aug" solves go
        through the solver's convergence monitor (include/asr_hip.h), each class stopping by itself once its loss has stalled.
        The result gains "sr_iters": {"aug": int32 [K'] numpy, the updates applied to each class of solved_ids} and in
        slice_max also {"aug_max": the same of the max maps' solves}; they are read back with the other results, after the
        whole image is enqueued.  The Adam bookkeeping does not change: every solve counts as num_iter steps, stopped or not.
        With sr_stop=None nothing else is launched and the result is what it was.

        sr_reweight ("cauchy", "hard" or {"kind": .., "kappa": .., "every": .., "start": ..}, any subset; check_sr_reweight): the
        "aug" solves down-weight whole unreliable copies (include/asr_hip.h, "copy reweighting"), on top of df_weights, per class.
        The result gains "copy_weights": {"aug": float32 [K', N] numpy, the final weight of every copy for each class of
        solved_ids} and in slice_max, whose max maps' solve is reweighted as well, also {"aug_max": the same of that solve}
        (under copy_dropout N counts the kept copies); read back with the other results.  With sr_reweight=None nothing else is
        launched and the result is what it was.

        couple (True needs Optimizer("primal_dual"); check_couple): the "aug" solve is ONE coupled solve over the solved classes
        (include/asr_hip.h, "multi-label coupling": x_k >= 0 and sum_k x_k <= 1 at every pixel; pruned classes are zero anyway, one
        class left is a group of 1; under sr_stop the classes stop together), and the "aug" map is ops.fuse_labels_simplex of its
        scores -- the class of largest share where that share exceeds the background's 1 - sum_k x_k, no threshold -- after the
        guided filter when guide is on; its counts are ops.class_counts'.  "max", "mean" and "standard" are untouched, and every
        other option works as it does without it.  Refused on the host before the model runs: modes slice and slice_max (their
        normalised stacks do not sum to at most 1), th_factors and crf (both read the threshold rule), an optimizer other than
        primal_dual.  With couple=False nothing else is launched and every result is what it was."""
        ids = [int(c) for c in class_ids]
        self.check_couple(couple, th_factors, crf)
        stop = self.check_sr_stop(sr_stop)
        reweight = self.check_sr_reweight(sr_reweight)
        if reweight is not None and getattr(self.sr, "verbose", False):
            raise ValueError("sr_reweight: the solver object is verbose (it cuts the solve into calls, where the weights would start over)")
        self.check_df_weights(df_weights)
        tv_beta = self.check_tv_guide(tv_guide, None if image_dev is None else tuple(image_dev.shape))
        crf_opts = self.check_crf(crf, None if image_dev is None else tuple(image_dev.shape), th_factors, len(ids))
        opts = self.label_options(None if image_dev is None else tuple(image_dev.shape), gt_dev is not None, band_widths,
                                  band_ignore_label, confusion_labels, th_factors, guide, coverages, keep_uncertainty,
                                  min_region, segments)
        if any(c == 0 for c in ids):
            raise ValueError(f"class id 0 is the fallback label, never a candidate: {ids}")
        unknown = [t for t in sr_types if t not in ("aug", "max", "mean")]
        if unknown:
            raise ValueError(f"sr_types may hold aug, max and mean, got {unknown}")
        sr_types = [t for t in ("aug", "max", "mean") if t in sr_types]
        if not sr_types and not want_standard:
            raise ValueError("no label map asked for: sr_types holds none of aug / max / mean and want_standard is False")
        starts = self._class_starts(ids, adam_starts)
        out_hw = self.sr.output_size
        keys = (["standard"] if want_standard else []) + sr_types
        maps = torch.empty((len(keys),) + tuple(out_hw), dtype=torch.int32, device=image_dev.device)
        classes = getattr(self.model, "classes", 0)

        def standard(logits0):
            ops.standard_labels(logits0, out_hw, ids, out=maps[0])

        conf = []                          # the copies' confidence stack [N, fh, fw], allocated from the first batch's logits

        def confidence(preds, first, k, n):
            if not conf:
                conf.append(torch.empty((n,) + tuple(preds.shape[1:3]), dtype=torch.float32, device=preds.device))
            # the confidence is taken from LOGITS: a model with a last_activation returns probabilities, and its raw logits
            # are the plan's buffer of this batch (as model.logits_of takes them for the standard output)
            activated = getattr(self.model, "last_activation", None) in ("softmax", "sigmoid")
            logits = self.model._raw_logits[:k] if activated else preds
            ops.opm_confidence(logits.contiguous(), df_weights, out=conf[0][first:first + k])

        y, ymax = self._classes_stage_model(image_dev, angles, shifts, ids, profile, standard if want_standard else None,
                                            confidence if df_weights is not None and "aug" in sr_types else None)
        kept = list(range(len(ids)))
        if prune and self.mode == "argmax":
            # raw argmax stacks hold ids[k] where the class wins and 0 elsewhere: a maximum of 0 is a class that never wins
            mx = ops.minmax(y, segments=len(ids))[:, 1].cpu().numpy()
            kept = [k for k in kept if mx[k] != 0.0]
            if len(kept) < len(ids):
                y = y[kept].contiguous() if kept else None
        solved = [ids[k] for k in kept]
        if kept:
            y, ymax = self._normalise(y, ymax)
        scores = {}
        sr_iters = {}                      # sr_stop: device int32 [K'] per solve, read back at the end
        copy_weights = {}                  # sr_reweight: device float32 [K', N] per solve, read back at the end
        fshifts = self._sr_frame(image_dev, shifts)
        with self._sr_stage_timed(profile):
            gt = self._gt_int32(gt_dev) if gt_dev is not None else None
            tally = (_LabelCounts(label_fields(keys, *opts.sizes, n_segments=opts.segments[0] if opts.segments else 0),
                                  image_dev.device) if gt is not None else None)
            f_dev = ops.to_device(opts.factors, device=image_dev.device) if opts.factors is not None and kept and sr_types else None
            g_image = None
            if crf_opts is not None or (opts.guide is not None and kept and sr_types):
                g_image = image_dev.to(torch.float32).contiguous()
            if crf_opts is not None and crf_opts.standard_conf is not None and want_standard:
                ops.crf_refine(g_image, ops.crf_unaries_from_labels(maps[0], ids, crf_opts.standard_conf), ids, crf_opts.params,
                               out=maps[0])
            if tally is not None and want_standard:
                tally.counts[0] = ops.class_counts(gt, maps[0])[0]
            g_state = None
            if opts.guide is not None and kept and sr_types:
                g_state = ops.guided_prepare(g_image, *opts.guide)
            tv_weights = None
            if tv_beta is not None and kept and "aug" in sr_types:
                tv_weights = ops.tv_edge_weights(image_dev.to(torch.float32).contiguous(), tv_beta)
            if kept:
                stop_kw = {} if stop is None else {"stop": stop, "iters": sr_iters}
                if couple:
                    stop_kw["couple"] = True
                if reweight is not None:
                    stop_kw.update(reweight=reweight, copy_weights=copy_weights)
                for t, tgt, tmax in self._classes_scores(y, ymax, angles, fshifts, [starts[k] for k in kept], sr_types,
                                                         tv_weights, conf[0] if conf else None, **stop_kw):
                    j = keys.index(t)
                    if g_state is not None:
                        ops.guided_apply(g_state, g_image, tgt, out=tgt)
                        if tmax is not None:
                            ops.guided_apply(g_state, g_image, tmax, out=tmax)
                    if couple and t == "aug":
                        ops.fuse_labels_simplex(tgt, solved, out=maps[j])
                        c = ops.class_counts(gt, maps[j])[0] if gt is not None else None
                    elif crf_opts is not None:
                        ops.crf_refine(g_image, ops.crf_unaries(tgt, self.th_factor, crf_opts.tau), solved, crf_opts.params,
                                       out=maps[j])
                        c = ops.class_counts(gt, maps[j])[0] if gt is not None else None
                    else:
                        _, c = ops.fuse_labels(tgt, solved, th_factor=self.th_factor, max_scores=tmax, truth=gt, out=maps[j],
                                               classes=classes)
                    if c is not None:
                        tally.counts[j] = c
                    if f_dev is not None:
                        ops.fuse_labels_sweep_counts(tgt, solved, gt, f_dev, classes=classes, out=tally.sweep[sr_types.index(t)])
                    if keep_scores:
                        scores[t] = (tgt, tmax)
            elif sr_types:
                first = keys.index(sr_types[0])
                maps[first:].zero_()
                if gt is not None:
                    tally.counts[first:] = ops.class_counts(gt, maps[first])[0]          # one count serves every (equal) zero map
                    if opts.factors is not None:
                        tally.sweep[:] = tally.counts[first]                             # ... under every factor
            self._advance_past(starts, adam_starts, sr_types)
            t_regions = ops.label_regions(gt.view(maps.shape[1:]), opts.segments[1]) if opts.segments is not None else None
            region_stats = (self._clean_label_maps(tally, gt, maps, opts.min_region, opts.segments, t_regions)
                            if opts.min_region is not None else None)
            if opts.segments is not None:
                self._match_segments(gt, maps, opts.segments, t_regions, None, tally.segments)
            u_map = self._score_label_maps(tally, gt, maps, opts, y if kept else None, angles, fshifts)
        res = {key: maps[j] for j, key in enumerate(keys)}
        res["solved_ids"] = solved
        if tally is not None:
            res.update(tally.to_host())
        elif region_stats is not None:
            host = region_stats.cpu().numpy()
            res["regions"] = {key: host[j] for j, key in enumerate(keys)}
        if keep_scores:
            res["scores"] = scores
        if stop is not None:
            res["sr_iters"] = {k: v.cpu().numpy() for k, v in sr_iters.items()}
        if reweight is not None:
            res["copy_weights"] = {k: v.cpu().numpy() for k, v in copy_weights.items()}
        if keep_uncertainty:
            res["uncertainty"] = u_map
            res["uncertainty_stacks"] = y if kept else None
        return res

    def check_couple(self, couple, th_factors=None, crf=None):
        """run_image_labels' couple, checked on the host before any launch: True needs the argmax mode (the normalised stacks
        of slice and slice_max do not sum to at most 1 over the classes), no th_factors and no crf (both read the threshold
        rule, which the coupled map does not have) and Optimizer("primal_dual").  ValueError otherwise."""
        if not isinstance(couple, (bool, np.bool_)):
            raise ValueError(f"couple must be True or False, got {couple!r}")
        if not couple:
            return
        if self.mode != "argmax":
            raise ValueError(f"couple in {self.mode} mode: the classes' normalised stacks do not sum to at most 1 there")
        if th_factors is not None:
            raise ValueError("th_factors with couple: the coupled label map has no threshold to sweep")
        if crf is not None:
            raise ValueError("crf with couple: the CRF's unaries are margins over the threshold rule, which the coupled map does not have")
        self.sr.check_couple()

    def check_df_weights(self, df_weights):
        """run_image_labels' df_weights, checked on the host before any launch: None, "maxprob" or "margin".  The confidence is
        made from the logits behind each forward batch: a model that both activates and upsamples its output (last_activation
        with final_upsample) keeps no logits at the size of the stacks and is refused."""
        if df_weights is not None and (not isinstance(df_weights, str) or df_weights not in _lib.CONF_KINDS):
            raise ValueError(f"df_weights must be None or one of {sorted(_lib.CONF_KINDS)}, got {df_weights!r}")
        if (df_weights is not None and getattr(self.model, "last_activation", None) in ("softmax", "sigmoid")
                and getattr(self.model, "final_upsample", False)):
            raise ValueError("df_weights needs the logits at the size of the stacks: the model applies a last_activation after "
                             "its final upsample (build it with final_upsample=False)")
        return df_weights

    def check_tv_guide(self, tv_guide, image_shape):
        """run_image_labels' tv_guide, checked on the host before any launch: None, or beta as a float.  ValueError for a beta
        that is not a finite number >= 0, an image that is not [H, W, 3] at the SR output size, and a bilateral-TV solver."""
        if tv_guide is None:
            return None
        beta = ops.check_tv_beta(tv_guide, "tv_guide")
        if image_shape != tuple(self.sr.output_size) + (3,):
            raise ValueError(f"tv_guide needs the image as [H, W, 3] at the SR output size {tuple(self.sr.output_size)}, got "
                             f"{image_shape}")
        if self.sr.use_BTV:
            raise ValueError("tv_guide: bilateral TV (use_BTV=True) has no edge-weighted form")
        return beta

    def check_crf(self, crf, image_shape, th_factors=None, num_ids=None):
        """run_image_labels' crf, checked on the host before any launch: None, or a CrfOptions (params: ops.CrfParams; tau;
        standard_conf | None).  ValueError for a bad field (ops.check_crf's wording), slice_max mode, th_factors next to it and an
        image that is not [H, W, 3] at the SR output size.  num_ids: the number of class ids, for standard_conf's range."""
        if crf is None:
            return None
        if not isinstance(crf, dict):
            raise ValueError(f"crf must be a dict of the CRF's fields, got {type(crf).__name__}")
        fields = dict(crf)
        tau = ops.check_crf_tau(fields.pop("tau", 0.1))
        conf = fields.pop("standard_conf", None)
        params = ops.check_crf(fields)
        if num_ids is not None and num_ids > ops.MAX_CRF_LABELS - 1:
            raise ValueError(f"crf: {num_ids} class ids above the cap of {ops.MAX_CRF_LABELS - 1} (label 0 and the ids make at most "
                             f"{ops.MAX_CRF_LABELS} labels)")
        if conf is not None:
            conf = ops.check_crf_conf(conf, (num_ids or 1) + 1)
        if self.mode == "slice_max":
            raise ValueError("crf in slice_max mode: a class passes against its max map there (S >= Smax), which is not a "
                             "threshold, so there is no unary")
        if th_factors is not None:
            raise ValueError("th_factors with crf: the sweep counts the fusion rule's label maps, not the CRF's")
        if image_shape != tuple(self.sr.output_size) + (3,):
            raise ValueError(f"crf needs the image as [H, W, 3] at the SR output size {tuple(self.sr.output_size)}, got "
                             f"{image_shape}")
        return CrfOptions(params, tau, conf)

    def label_options(self, image_shape, has_gt, band_widths=None, band_ignore_label=255, confusion_labels=None,
                      th_factors=None, guide=None, coverages=None, keep_uncertainty=False, min_region=None, segments=None):
        """The scoring options of run_image_labels, checked and normalised into one LabelOptions; ValueError as its docstring
        says.  Host only, and nothing of self is read that the options given do not need (mode: th_factors; sr: guide).
        image_shape: the image's shape or None; has_gt: a ground truth comes with it."""
        covs = ops.check_coverages(coverages) if coverages is not None else None
        if covs is not None and not has_gt:
            raise ValueError("coverages needs gt_dev: the risk-coverage curve scores the label maps against a ground truth")
        if keep_uncertainty and covs is None:
            raise ValueError("keep_uncertainty without coverages: the uncertainty map is only built for the risk-coverage curve")
        if guide is not None:
            try:
                g_radius, g_eps = guide
            except (TypeError, ValueError):
                raise ValueError(f"guide must be (radius, eps), got {guide!r}") from None
            guide = ops.check_guided(g_radius, g_eps)
            if image_shape != tuple(self.sr.output_size) + (3,):
                raise ValueError(f"guide needs the image as [H, W, 3] at the SR output size {tuple(self.sr.output_size)}, got "
                                 f"{image_shape}")
        if min_region is not None:
            min_region = ops.check_min_region(min_region)
            if th_factors is not None:
                raise ValueError("th_factors with min_region: the sweep counts label maps that are never written, so there is "
                                 "nothing to clean")
        if segments is not None:
            segments = ops.check_segments(segments)
            if not has_gt:
                raise ValueError("segments needs gt_dev: the segments of a label map are matched against those of a ground truth")
            if th_factors is not None:
                raise ValueError("th_factors with segments: the sweep counts label maps that are never written, so there are no "
                                 "segments to match")
        factors = None
        if th_factors is not None:
            if not has_gt:
                raise ValueError("th_factors needs gt_dev: the sweep counts every factor's label map against a ground truth")
            if self.mode == "slice_max":
                raise ValueError("th_factors in slice_max mode: a class passes against its max map there, the threshold plays no "
                                 "part, so there is nothing to sweep")
            factors = np.asarray(th_factors, dtype=np.float32).reshape(-1)
            if not 1 <= factors.size <= ops.MAX_LABEL_SWEEP_FACTORS:
                raise ValueError(f"{factors.size} threshold factors (1..{ops.MAX_LABEL_SWEEP_FACTORS})")
        bands = ops.check_band_widths(band_widths) if band_widths is not None else None
        n_conf = ops.check_confusion_labels(confusion_labels) if confusion_labels is not None else 0
        if n_conf and not has_gt:
            raise ValueError("confusion_labels needs gt_dev: a confusion matrix is counted against a ground truth")
        band_ignore = -1 if bands is None or band_ignore_label is None else int(band_ignore_label)
        sizes = (len(bands or ()), n_conf, 0 if factors is None else factors.size, len(covs or ()), int(min_region is not None))
        return LabelOptions(bands, band_ignore, n_conf, factors, guide, covs, sizes, min_region, segments)

    @staticmethod
    def _match_segments(gt, maps, segments, truth_regions, pred_regions, out):
        """ops.segment_match of the label maps [M, H, W] against gt into out [M, L, 4]; pred_regions None: labelled here."""
        num_labels, connectivity, include_zero = segments
        ops.segment_match(gt.view(maps.shape[1:]), maps, num_labels, connectivity, include_zero, truth_regions=truth_regions,
                          pred_regions=pred_regions, out=out)

    @staticmethod
    def _clean_label_maps(tally, gt, maps, min_region, segments=None, truth_regions=None):
        """The small regions of the finished label maps [M, H, W] removed in place (one labelling and one clean-up call over
        all of them); with a tally the raw counts kept, the counts taken again on the cleaned maps and the region statistics
        stored.  With segments the maps are matched against the truth before they change (tally.raw_segments), on the
        clean-up's own labelling when the connectivities agree.  Returns the statistics, device int64 [M, 4]."""
        min_area, connectivity = min_region
        regions = ops.label_regions(maps, connectivity)
        if segments is not None:
            HotPath._match_segments(gt, maps, segments, truth_regions, regions if segments[1] == connectivity else None,
                                    tally.raw_segments)
        _, stats = ops.clean_labels(maps, min_area, connectivity, regions=regions, out=maps, want_stats=True)
        if tally is not None:
            tally.raw[:] = tally.counts
            for j in range(maps.shape[0]):
                tally.counts[j] = ops.class_counts(gt, maps[j])[0]
            tally.regions[:] = stats
        return stats

    def _score_label_maps(self, tally, gt, maps, opts, stacks, angles, fshifts):
        """The scores of the finished label maps [M, H, W] against gt, into tally: trimap bands, confusion matrices, risk-coverage
        (stacks: the [K', N, h, w] class stacks the solver read, None when no class was solved).  Returns the uncertainty map,
        None without coverages."""
        out_hw = tuple(maps.shape[1:])
        if opts.bands is not None and gt is not None:
            r_max = max(opts.bands)
            ops.band_class_counts(gt, maps, ops.boundary_dist2(gt.view(out_hw), r_max), opts.bands, r_max, opts.band_ignore,
                                  out=tally.band)
        if opts.n_conf:
            ops.confusion_counts(gt, maps, opts.n_conf, out=tally.confusion)
        if opts.covs is None:
            return None
        u_map = self._uncertainty(stacks, angles, fshifts, out_hw, maps.device)
        edges = coverage_edges(u_map, gt, opts.covs, ignore_label=255)
        ops.binned_class_counts(gt, maps, u_map, edges, ignore_label=255, out=tally.coverage)
        tally.retained[:] = coverage_retained(u_map, gt, edges, ignore_label=255)
        return u_map

    def _uncertainty(self, y, angles, fshifts, out_hw, device):
        """utils.uncertainty_map of the class stacks y [K', N, h, w] (None: no class): one moments launch under frame coverage."""
        if y is None:
            return torch.full(tuple(out_hw), float("inf"), dtype=torch.float32, device=device)
        a = np.repeat(np.asarray(angles, dtype=np.float32)[None], y.shape[0], axis=0)
        s = np.repeat(np.asarray(fshifts, dtype=np.float32)[None], y.shape[0], axis=0)
        rot, tr = self.sr._transforms(a, s, y.device, negate=True)
        ones = torch.ones(tuple(y.shape[2:]), dtype=torch.float32, device=y.device)
        mom = ops.realign_moments(y, tr, rot, out_hw, want=("var", "nv"), wgt=ones, valid_min=0.5)
        return uncertainty_map(mom["var"], mom["nv"], opm_scales(range(y.shape[0]), self.mode, normalised=True))

    def _finish(self, res):
        res.pop("_masks", None)          # the rows stay alive through the per-key views
        if "_iou_counts" in res:
            res["ious"] = self._ious_from_counts(res.pop("_iou_keys"), res.pop("_iou_counts").cpu().numpy())
        return res

    def _iou_counts(self, res, gt_dev):
        """Integer intersection / union counts of every produced mask against the ground truth (device): one launch over
        the image's mask buffer; rows of masks that were not asked for are ignored."""
        keys = [k for k in self.MASK_KEYS if k in res]
        rows = [self.MASK_KEYS.index(k) for k in keys]
        masks = res["_masks"]
        if rows != list(range(len(self.MASK_KEYS))):                    # a subset of the four masks: compact it
            masks = masks[rows].contiguous()
        return keys, ops.iou_counts_shared_truth(self._gt_int32(gt_dev), masks, self.class_id, include_bg=True)

    @staticmethod
    def _ious_from_counts(keys, counts):
        """[standard_single, standard_bg, aug_single, aug_bg, max, mean] (SR_single_class.py:109-120)."""
        by = dict(zip(keys, counts))
        nan = float("nan")

        def iou(k, bg):
            return iou_from_counts(by[k], bg) if k in by else nan

        return np.array([iou("standard", False), iou("standard", True), iou("aug", False), iou("aug", True),
                         iou("max", False), iou("mean", False)], dtype=np.float64)


# HotPath.label_options' value: band widths | None and the label left out of the bands (-1: none), confusion labels (0: off),
# float32 threshold factors | None, the guide's (radius, eps) | None, coverages | None; sizes: (B, L, T, C, R), 0 where off (R: 1
# with min_region); min_region: (min_area, connectivity) | None; segments: (num_labels, connectivity, include_zero) | None
# HotPath.check_crf's value: ops.CrfParams, the unaries' tau, the standard map's conf | None (left alone)
CrfOptions = namedtuple("CrfOptions", "params tau standard_conf")
LabelOptions = namedtuple("LabelOptions", "bands band_ignore n_conf factors guide covs sizes min_region segments")


class _LabelCounts:
    """The counts of run_image_labels on the device, one int64 allocation so that they reach the host in one copy: the fields
    of label_record.label_layout one after another; after them, with C coverages, C + 1 pixel totals (the counted pixels each
    coverage retained, then all of them).  Each field that is on is the attribute of its prefix's name -- counts, band,
    confusion, sweep, coverage, raw, regions, segments, raw_segments -- as [len(keys), *shape]: what the ops.*_counts(out=...) call of that score writes into."""

    def __init__(self, fields, device):
        spans, end = label_layout(fields, with_miou=False)
        self._fields = [(f, at) for f, (_, at) in zip(fields, spans)]
        n_cov = next((f.shape[0] for f in fields if f.prefix == "coverage_"), 0)
        self._buf = torch.empty(end + (n_cov + 1 if n_cov else 0), dtype=torch.int64, device=device)
        for f, at in self._fields:
            setattr(self, f.prefix.rstrip("_") or "counts", self._buf[at].view((len(f.keys),) + f.shape))
        self.retained = self._buf[end:]                         # [C + 1]: utils.coverage_retained

    def to_host(self):
        """The count and Mean_IOU entries of the result, by field, and with coverages "coverage_share"."""
        host = self._buf.cpu().numpy()
        res = {}
        for f, at in self._fields:
            counts = host[at].reshape((len(f.keys),) + f.shape)
            res[counts_name(f)] = {key: counts[j] for j, key in enumerate(f.keys)}
            if f.scored:
                miou = np.array([mean_iou_from_counts(c) for c in counts.reshape(-1, 3, 256)], dtype=np.float64)
                miou = miou.reshape((len(f.keys),) + f.shape[:-2])
                res[f.prefix + "Mean_IOU"] = {key: miou[j] if miou[j].ndim else float(miou[j]) for j, key in enumerate(f.keys)}
        if self.retained.numel():
            ret = host[-self.retained.numel():]
            with np.errstate(divide="ignore", invalid="ignore"):
                res["coverage_share"] = np.float64(ret[:-1]) / np.float64(ret[-1])
        return res


class _Pending:
    """Handle of an image whose SR stage is still running on the side stream."""

    def __init__(self, path, res, done, keep):
        self._path, self._res, self._done, self._keep = path, res, done, keep

    def result(self):
        self._done.synchronize()
        self._keep = None
        return self._path._finish(self._res)
