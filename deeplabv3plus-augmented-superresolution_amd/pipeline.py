"""The whole hot path for one image, device-resident end to end:

    augment (N copies) -> DeepLabV3+ forward -> OPM -> {ASR solve, max-SR, mean-SR} -> threshold
    -> IoU counts

i.e. the body of test_SR.py:73-94 / generate_augmented_copies.py:88-91 + SR_single_class.py:83-127
without the host round trips (ndarray lists, HDF5) the reference puts between the stages.
Used by bench.py, the scripts and the smoke test.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .superresolution_scripts import augmentation_utils as au
from .utils import iou_from_counts, mean_iou_from_counts


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

    # ---- stage 1 (model stream): augment -> forward -> OPM (-> standard mask) --------------------------
    def _stage_model(self, image_dev, angles, shifts, profile=None, want_standard=True, lane=0):
        """The copies go through the model one forward batch at a time (augmentation_utils.py:30-59 draws them in chunks
        for the same reason): each batch is augmented straight into the plan's input buffer, its logits are consumed in
        place by the OPM kernel, which writes its rows of the image's [N,h,w] stack -- nothing of size [N,H,W,3] or
        [N,h,w,classes] outlives a batch."""
        out_hw = self.sr.output_size
        n = len(angles)
        h, w, _ = image_dev.shape
        eng = self.model.engine
        bs = min(self.batch_size, n)
        y = ymax = None                     # [1, N, fh, fw], allocated from the first batch's logits: their size depends on the
        res = {"_masks": torch.empty((len(self.MASK_KEYS),) + tuple(out_hw), dtype=torch.int32, device=image_dev.device)}
        for i in range(0, n, bs):
            k = min(bs, n - i)
            copies = au.augment_on_device(image_dev, angles[i:i + k], shifts[i:i + k], out=eng.input_view(k, h, w, lane))
            preds = self.model.predict_device(copies, batch_size=k, profile=profile, lane=lane, clone=False)  # logits stay there
            if y is None:                   # decoder / upsampling options, not only on the backbone's stride
                y = torch.empty((1, n) + tuple(preds.shape[1:3]), dtype=torch.float32, device=image_dev.device)
                ymax = torch.empty_like(y) if self.mode == "slice_max" else None
            if i == 0 and want_standard:
                res["standard"] = self.standard_mask(self.model.logits_of(preds, 0), out_hw, out=res["_masks"][0])
            au.output_processing(preds, self.class_id, self.mode, out=y[0, i:i + k],
                                 out_max=ymax[0, i:i + k] if ymax is not None else None)
            del copies, preds
        if self.mode != "slice":            # load_SR_data's global min-max normalisation (superres_utils.py:183-192)
            y = self._normalise(y)
            if ymax is not None:
                ymax = self._normalise(ymax)
        return res, y, ymax

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
    def _stage_sr(self, res, y, ymax, angles, shifts, gt_dev, adam_start, sr_types):
        sr = self.sr
        a, s = angles[None], shifts[None]
        both = None
        if "max" in sr_types and "mean" in sr_types:            # one pass over the copies serves both (bit-identical)
            both = (sr.realign_batch(y, a, s, "both"), sr.realign_batch(ymax, a, s, "both") if ymax is not None else None)
        for t in sr_types:
            if t == "aug":
                if adam_start is not None:
                    sr.optimizer.optimizer.iterations = adam_start
                tgt, _ = sr.augmented_superresolution_batch(y, a, s)
                tmax = sr.augmented_superresolution_batch(ymax, a, s)[0] if ymax is not None else None
            elif both is not None:
                k = 0 if t == "max" else 1
                tgt, tmax = both[0][k], (both[1][k] if both[1] is not None else None)
            else:
                tgt = sr.realign_batch(y, a, s, t)
                tmax = sr.realign_batch(ymax, a, s, t) if ymax is not None else None
            res[t] = self._threshold(tgt[0], tmax[0] if tmax is not None else None,
                                     out=res["_masks"][self.MASK_KEYS.index(t)])
        if gt_dev is not None:
            res["_iou_keys"], res["_iou_counts"] = self._iou_counts(res, gt_dev)
        return res

    def run_image(self, image_dev, angles, shifts, gt_dev=None, adam_start=None, profile=None,
                  sr_types=("aug", "max", "mean"), want_standard=True):
        """image_dev [H,W,3] float32 device; angles [N], shifts [N,2] float32 host arrays;
        gt_dev [H,W] int32 device labels (optional).  Returns dict of device masks (+ 6 IoUs)."""
        res, y, ymax = self._stage_model(image_dev, angles, shifts, profile, want_standard)
        if profile is not None:         # the SR stage (solve, realign, thresholds, IoU counts) as one HIP-event interval
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        res = self._stage_sr(res, y, ymax, angles, self._sr_frame(image_dev, shifts), gt_dev, adam_start, sr_types)
        if profile is not None:
            e1.record()
            torch.cuda.synchronize()
            profile["_sr_stage_ms"] = profile.get("_sr_stage_ms", 0.0) + e0.elapsed_time(e1)
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
    def _class_starts(self, ids, adam_starts):
        """Global Adam step counter before each class's solve: adam_starts[c], or consecutive solves in the order of ids
        from the current counter."""
        sr = self.sr
        solves = 2 if self.mode == "slice_max" else 1
        if adam_starts is None:
            it0 = sr.optimizer.optimizer.iterations if sr.optimizer is not None else 0
            return [it0 + j * solves * sr.num_iter for j in range(len(ids))]
        return [int(adam_starts[c]) for c in ids]

    def _classes_stage_model(self, image_dev, angles, shifts, ids, profile, standard):
        """Stage 1 of a class set: augment -> forward per batch -> OPM of every class into raw [K, N, h, w] stacks (y, ymax).
        standard: None, or a function of copy 0's logits [h, w, C] (the standard masks / label map are made from them)."""
        k_set = len(ids)
        n = len(angles)
        h, w, _ = image_dev.shape
        eng = self.model.engine
        bs = min(self.batch_size, n)
        y = ymax = None
        for i in range(0, n, bs):
            k = min(bs, n - i)
            copies = au.augment_on_device(image_dev, angles[i:i + k], shifts[i:i + k], out=eng.input_view(k, h, w, 0))
            preds = self.model.predict_device(copies, batch_size=k, profile=profile, clone=False)
            if y is None:
                y = torch.empty((k_set, n) + tuple(preds.shape[1:3]), dtype=torch.float32, device=image_dev.device)
                ymax = torch.empty_like(y) if self.mode == "slice_max" else None
            if i == 0 and standard is not None:
                standard(self.model.logits_of(preds, 0).contiguous())
            au.output_processing_classes(preds, ids, self.mode, out=y[:, i:i + k],
                                         out_max=ymax[:, i:i + k] if ymax is not None else None)
            del copies, preds
        return y, ymax

    def _classes_normalise(self, y, ymax):
        """load_SR_data's normalisation, per class stack (not in slice mode)."""
        if self.mode != "slice":
            k_set = y.shape[0]
            y = ops.minmax_normalize(y, segments=k_set, new_min=0.0, new_max=1.0)
            if ymax is not None:
                ymax = ops.minmax_normalize(ymax, segments=k_set, new_min=0.0, new_max=1.0)
        return y, ymax

    def _classes_scores(self, y, ymax, angles, fshifts, starts, sr_types):
        """Stage 2 of a class set up to the SR outputs: yields (t, scores [K, H, W], max-map scores [K, H, W] | None) for each
        SR type, the K classes as a batch of the existing solver / realign."""
        sr = self.sr
        k_set = y.shape[0]
        a = np.repeat(np.asarray(angles, dtype=np.float32)[None], k_set, axis=0)
        s = np.repeat(np.asarray(fshifts, dtype=np.float32)[None], k_set, axis=0)
        both = None
        if "max" in sr_types and "mean" in sr_types:
            both = (sr.realign_batch(y, a, s, "both"), sr.realign_batch(ymax, a, s, "both") if ymax is not None else None)
        for t in sr_types:
            if t == "aug":
                tgt, _ = sr.augmented_superresolution_classes(y, angles, fshifts, starts)
                tmax = (sr.augmented_superresolution_classes(ymax, angles, fshifts, [st + sr.num_iter for st in starts])[0]
                        if ymax is not None else None)
            elif both is not None:
                j = 0 if t == "max" else 1
                tgt, tmax = both[0][j], (both[1][j] if both[1] is not None else None)
            else:
                tgt = sr.realign_batch(y, a, s, t)
                tmax = sr.realign_batch(ymax, a, s, t) if ymax is not None else None
            yield t, tgt, tmax

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
        k_set = len(ids)
        sr = self.sr
        solves = 2 if self.mode == "slice_max" else 1
        starts = self._class_starts(ids, adam_starts)
        # stage 1: augment -> forward per batch -> OPM of every class into [K, N, h, w] stacks
        out_hw = sr.output_size
        masks = torch.empty((len(self.MASK_KEYS), k_set) + tuple(out_hw), dtype=torch.int32, device=image_dev.device)
        have = []

        def standard(logits0):
            ops.standard_mask_classes(logits0, out_hw, ids, out=masks[0])
            have.append("standard")

        y, ymax = self._classes_stage_model(image_dev, angles, shifts, ids, profile, standard if want_standard else None)
        y, ymax = self._classes_normalise(y, ymax)
        # stage 2: the K classes as a batch of the existing solver / realign, then K-class threshold and IoU counts
        if profile is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        for t, tgt, tmax in self._classes_scores(y, ymax, angles, self._sr_frame(image_dev, shifts), starts, sr_types):
            row = masks[self.MASK_KEYS.index(t)]
            if tmax is not None:
                ops.threshold_classes(tgt, ids, th_mask=tmax, out=row)
            else:
                ops.threshold_classes(tgt, ids, th_factor=self.th_factor, out=row)
            have.append(t)
        if adam_starts is None and "aug" in sr_types and sr.optimizer is not None:
            sr.optimizer.optimizer.iterations = starts[-1] + solves * sr.num_iter
        keys = [key for key in self.MASK_KEYS if key in have]
        counts = None
        if gt_dev is not None:
            gt = gt_dev if gt_dev.dtype == torch.int32 else gt_dev.to(torch.int32)
            preds = masks[[self.MASK_KEYS.index(key) for key in keys]].transpose(0, 1).contiguous()     # [K, M, H, W]
            counts = ops.iou_counts_classes(gt.contiguous(), preds, ids, include_bg=True)
        if profile is not None:
            e1.record()
            torch.cuda.synchronize()
            profile["_sr_stage_ms"] = profile.get("_sr_stage_ms", 0.0) + e0.elapsed_time(e1)
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
                         band_widths=None, band_ignore_label=255):
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
        With band_widths=None nothing else is launched and nothing else returned."""
        ids = [int(c) for c in class_ids]
        bands = ops.check_band_widths(band_widths) if band_widths is not None else None
        if any(c == 0 for c in ids):
            raise ValueError(f"class id 0 is the fallback label, never a candidate: {ids}")
        unknown = [t for t in sr_types if t not in ("aug", "max", "mean")]
        if unknown:
            raise ValueError(f"sr_types may hold aug, max and mean, got {unknown}")
        sr_types = [t for t in ("aug", "max", "mean") if t in sr_types]
        if not sr_types and not want_standard:
            raise ValueError("no label map asked for: sr_types holds none of aug / max / mean and want_standard is False")
        sr = self.sr
        solves = 2 if self.mode == "slice_max" else 1
        starts = self._class_starts(ids, adam_starts)
        out_hw = sr.output_size
        dev = image_dev.device
        keys = (["standard"] if want_standard else []) + sr_types
        maps = torch.empty((len(keys),) + tuple(out_hw), dtype=torch.int32, device=dev)
        classes = getattr(self.model, "classes", 0)

        def standard(logits0):
            ops.standard_labels(logits0, out_hw, ids, out=maps[0])

        y, ymax = self._classes_stage_model(image_dev, angles, shifts, ids, profile, standard if want_standard else None)
        kept = list(range(len(ids)))
        if prune and self.mode == "argmax":
            # raw argmax stacks hold ids[k] where the class wins and 0 elsewhere: a maximum of 0 is a class that never wins
            mx = ops.minmax(y, segments=len(ids))[:, 1].cpu().numpy()
            kept = [k for k in kept if mx[k] != 0.0]
            if len(kept) < len(ids):
                y = y[kept].contiguous() if kept else None
        solved = [ids[k] for k in kept]
        if kept:
            y, ymax = self._classes_normalise(y, ymax)
        if profile is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        gt = None
        counts = None
        if gt_dev is not None:
            gt = (gt_dev if gt_dev.dtype == torch.int32 else gt_dev.to(torch.int32)).contiguous()
            if bands is None:
                counts = torch.empty((len(keys), 3, 256), dtype=torch.int64, device=dev)
            else:                                   # one buffer for both sets of counts: they reach the host in one copy
                both = torch.empty(len(keys) * (1 + len(bands)) * 768, dtype=torch.int64, device=dev)
                counts = both[:len(keys) * 768].view(len(keys), 3, 256)
            if want_standard:
                counts[0] = ops.class_counts(gt, maps[0])[0]
        scores = {}
        if kept:
            for t, tgt, tmax in self._classes_scores(y, ymax, angles, self._sr_frame(image_dev, shifts),
                                                     [starts[k] for k in kept], sr_types):
                j = keys.index(t)
                _, c = ops.fuse_labels(tgt, solved, th_factor=self.th_factor, max_scores=tmax, truth=gt, out=maps[j],
                                       classes=classes)
                if c is not None:
                    counts[j] = c
                if keep_scores:
                    scores[t] = (tgt, tmax)
        elif sr_types:
            first = keys.index(sr_types[0])
            maps[first:].zero_()
            if gt is not None:
                counts[first:] = ops.class_counts(gt, maps[first])[0]          # one count serves every (equal) zero map
        if adam_starts is None and "aug" in sr_types and sr.optimizer is not None and ids:
            sr.optimizer.optimizer.iterations = starts[-1] + solves * sr.num_iter
        if bands is not None and gt is not None:
            r_max = max(bands)
            ops.band_class_counts(gt, maps, ops.boundary_dist2(gt.view(out_hw[0], out_hw[1]), r_max), bands, r_max,
                                  -1 if band_ignore_label is None else int(band_ignore_label), out=both[len(keys) * 768:])
        if profile is not None:
            e1.record()
            torch.cuda.synchronize()
            profile["_sr_stage_ms"] = profile.get("_sr_stage_ms", 0.0) + e0.elapsed_time(e1)
        res = {key: maps[j] for j, key in enumerate(keys)}
        res["solved_ids"] = solved
        if counts is not None and bands is not None:
            host = both.cpu().numpy()
            band = host[len(keys) * 768:].reshape(len(keys), len(bands), 3, 256)
            host = host[:len(keys) * 768].reshape(len(keys), 3, 256)
            res["band_counts"] = {key: band[j] for j, key in enumerate(keys)}
            res["band_Mean_IOU"] = {key: np.array([mean_iou_from_counts(c) for c in band[j]], dtype=np.float64)
                                    for j, key in enumerate(keys)}
        elif counts is not None:
            host = counts.cpu().numpy()
        if counts is not None:
            res["counts"] = {key: host[j] for j, key in enumerate(keys)}
            res["Mean_IOU"] = {key: mean_iou_from_counts(host[j]) for j, key in enumerate(keys)}
        if keep_scores:
            res["scores"] = scores
        return res

    def _finish(self, res):
        res.pop("_masks", None)          # the rows stay alive through the per-key views
        if "_iou_counts" in res:
            res["ious"] = self._ious_from_counts(res.pop("_iou_keys"), res.pop("_iou_counts").cpu().numpy())
        return res

    @staticmethod
    def _normalise(stack):
        """load_SR_data's global min-max normalisation of an image's masks to [0, 1] (superres_utils.py:183-206)."""
        return ops.minmax_normalize(stack.contiguous(), segments=1, new_min=0.0, new_max=1.0)

    def _iou_counts(self, res, gt_dev):
        """Integer intersection / union counts of every produced mask against the ground truth (device): one launch over
        the image's mask buffer; rows of masks that were not asked for are ignored."""
        keys = [k for k in self.MASK_KEYS if k in res]
        rows = [self.MASK_KEYS.index(k) for k in keys]
        masks = res["_masks"]
        if rows != list(range(len(self.MASK_KEYS))):                    # a subset of the four masks: compact it
            masks = masks[rows].contiguous()
        gt = gt_dev if gt_dev.dtype == torch.int32 else gt_dev.to(torch.int32)
        return keys, ops.iou_counts_shared_truth(gt.contiguous(), masks, self.class_id, include_bg=True)

    @staticmethod
    def _ious_from_counts(keys, counts):
        """[standard_single, standard_bg, aug_single, aug_bg, max, mean] (SR_single_class.py:109-120)."""
        by = dict(zip(keys, counts))
        nan = float("nan")

        def iou(k, bg):
            return iou_from_counts(by[k], bg) if k in by else nan

        return np.array([iou("standard", False), iou("standard", True), iou("aug", False), iou("aug", True),
                         iou("max", False), iou("mean", False)], dtype=np.float64)


class _Pending:
    """Handle of an image whose SR stage is still running on the side stream."""

    def __init__(self, path, res, done, keep):
        self._path, self._res, self._done, self._keep = path, res, done, keep

    def result(self):
        self._done.synchronize()
        self._keep = None
        return self._path._finish(self._res)
