"""SR glue with the reference's surface (superresolution_scripts/superres_utils.py):
``min_max_normalization`` (:56-62), ``threshold_image`` (:118-139), ``load_SR_data`` (:154-210),
``compute_SR`` (:213-273) and ``check_hdf5_validity`` (:108-115), plus the thin host-side list helpers the reference's
scripts import from this module (``get_img_paths`` :9-29, ``class_in_image`` :32-38, ``filter_images_by_class`` :41-53,
``load_precomputed_images`` :65-78, ``get_precomputed_folders_path`` :81-90, ``list_precomputed_data_paths`` :93-105,
``normalize_coefficients`` :142-151): pure file plumbing, no device work, kept so that code written against the
reference's module still imports.  The interchange file is the reference's HDF5 file (same dataset and
attribute names, written / read by ``hdf5_lite``: files from the reference's h5py writer load here and vice versa);
an ``.npz`` with the same keys is accepted too (``ASR_DATA_EXT=.npz`` makes it the written format).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _lib, hdf5_lite, ops

DATA_EXT = os.environ.get("ASR_DATA_EXT", ".hdf5")          # what save_SR_data writes: ".hdf5" (reference) or ".npz"
DATA_EXTS = (".hdf5", ".h5", ".npz")                         # what the readers accept


# ---- list helpers (host only) ------------------------------------------------------------------------
def _stem_as_int(path):
    return int(os.path.basename(path).split(".")[0])


def get_img_paths(image_list_path, image_folder, is_png=False, sort=True):
    """One image id per line of ``image_list_path`` -> ``image_folder/<id>.jpg`` (``.png`` with is_png); ``sort`` orders
    the result by the integer value of the id (VOC ids are integers)."""
    suffix = ".png" if is_png else ".jpg"
    with open(image_list_path) as fh:
        ids = [line.rstrip() for line in fh]
    paths = [os.path.join(image_folder, i + suffix) for i in ids]
    return sorted(paths, key=_stem_as_int) if sort else paths


def class_in_image(image_path, class_id, image_size=(512, 512)):
    """Does the label map that belongs to ``image_path`` (same VOC tree: JPEGImages -> SegmentationClassAug, jpg -> png)
    contain ``class_id``?  The map is resized with nearest neighbour like every label map of the path."""
    from ..utils import load_image
    label_path = image_path.replace("JPEGImages", "SegmentationClassAug").replace("jpg", "png")
    labels = load_image(label_path, image_size=image_size, normalize=False, is_png=True, resize_method="nearest")
    return bool((np.asarray(labels) == class_id).any())


def filter_images_by_class(path_list, filter_class_id, num_images=None, image_size=(512, 512)):
    """The paths whose label map contains ``filter_class_id``, in list order, at most ``num_images`` of them."""
    limit = len(path_list) if num_images is None else num_images
    kept = []
    for path in path_list:
        if len(kept) == limit:
            break
        if class_in_image(path, class_id=filter_class_id, image_size=image_size):
            kept.append(path)
    return kept


def load_precomputed_images(img_folder):
    """The PNG copies ``0.png, 1.png, ...`` of a pre-HDF5 output folder, in numeric order (its ``.npy`` side files are
    not images)."""
    from ..utils import load_image
    numbers = sorted(int(name[:-len(".png")]) for name in os.listdir(img_folder) if ".npy" not in name)
    return [load_image(os.path.join(img_folder, f"{k}.png"), normalize=False, is_png=True) for k in numbers]


def get_precomputed_folders_path(root_dir, num_aug=100):
    """Sub-folders of ``root_dir`` that are complete: ``num_aug`` copies plus the two side files (angles, shifts).
    Incomplete ones are reported and left out."""
    complete = []
    for name in os.listdir(root_dir):
        folder = os.path.join(root_dir, name)
        if len(os.listdir(folder)) != num_aug + 2:
            print(f"Skipped folder named {name} as it is not valid")
            continue
        complete.append(folder)
    return complete


def list_precomputed_data_paths(root_dir, sort=False):
    """Every ``.hdf5`` interchange file below ``root_dir`` (os.walk order, or by integer stem with ``sort``).  The
    evaluation loop of this package uses ``asr_amd.evaluation.interchange_files`` instead: one order on every rank,
    ``.npz`` files too, one file per stem."""
    found = [os.path.join(folder, f) for folder, _dirs, files in os.walk(root_dir) for f in files if f.endswith(".hdf5")]
    return sorted(found, key=_stem_as_int) if sort else found


def normalize_coefficients(coeff_dict):
    """The same keys with the values scaled to sum to one."""
    total = np.sum(list(coeff_dict.values()))
    return {key: value / total for key, value in coeff_dict.items()}


def min_max_normalization(image, new_min=0.0, new_max=255.0, global_min=None, global_max=None):
    """Host arrays: numpy float32 arithmetic in the reference's order.  Device tensors stay on the device."""
    if isinstance(image, torch.Tensor) and image.is_cuda:
        mm = ops.minmax(image.contiguous())[0]
        mn = mm[0] if global_min is None else torch.as_tensor(global_min, dtype=torch.float32, device=image.device)
        mx = mm[1] if global_max is None else torch.as_tensor(global_max, dtype=torch.float32, device=image.device)
        den = mx - mn
        den = torch.where(den != 0, den, torch.ones_like(den))
        return new_min + ((image - mn) * (new_max - new_min)) / den
    image = np.asarray(image)
    mn = image.min() if global_min is None else global_min
    mx = image.max() if global_max is None else global_max
    num = (image - mn) * (new_max - new_min)
    den = (mx - mn) if (mx - mn) != 0 else 1.0
    return new_min + (num / den)


def threshold_image(image, th_value, th_factor=.15, th_mask=None):
    """{0, th_value} int32 mask: image >= th_mask, or image > th_factor * max(image).  Runs on the
    device (asr_threshold_f32); returns a host array for host input, a device tensor otherwise."""
    was_tensor = isinstance(image, torch.Tensor)
    dev = _lib.require_gpu()
    img = image if was_tensor else torch.as_tensor(np.asarray(image, dtype=np.float32))
    img = img.to(device=dev, dtype=torch.float32).contiguous()
    tm = None
    if th_mask is not None:
        tm = th_mask if isinstance(th_mask, torch.Tensor) else torch.as_tensor(np.asarray(th_mask, dtype=np.float32))
        tm = tm.to(device=dev, dtype=torch.float32).contiguous()
    out = ops.threshold(img, th_value, th_factor=th_factor, th_mask=tm)
    return out if was_tensor else out.cpu().numpy()


def guided_refine(image, guide, radius=8, eps=1e-3):
    """The guided filter of include/asr_hip.h on a score map: ``image`` [H, W], [H, W, 1] or [P, H, W] float32 refined against
    the colour ``guide`` [H, W, 3] (the RGB image at the score map's size, values in [0, 1]), same shape out.  It moves the
    boundary of an upsampled score map onto the image's own edges before the map is thresholded.  Runs on the device
    (ops.guided_filter); returns a host array for a host ``image``, a device tensor otherwise."""
    was_tensor = isinstance(image, torch.Tensor)
    radius, eps = ops.check_guided(radius, eps)
    g = guide if isinstance(guide, torch.Tensor) else torch.as_tensor(np.asarray(guide, dtype=np.float32))
    if g.dim() != 3 or g.shape[2] != 3:
        raise ValueError(f"guided_refine: the guide must be [H, W, 3], got {tuple(g.shape)}")
    H, W = int(g.shape[0]), int(g.shape[1])
    img = image if was_tensor else torch.as_tensor(np.asarray(image, dtype=np.float32))
    shape = tuple(img.shape)
    if shape not in ((H, W), (H, W, 1)) and not (len(shape) == 3 and shape[0] >= 1 and shape[1:] == (H, W)):
        raise ValueError(f"guided_refine: image must be [{H}, {W}], [{H}, {W}, 1] or [P, {H}, {W}], got {shape}")
    dev = _lib.require_gpu()
    g = g.to(device=dev, dtype=torch.float32).contiguous()
    img = img.to(device=dev, dtype=torch.float32).contiguous()
    planes = img.reshape(1, H, W) if shape in ((H, W), (H, W, 1)) else img
    out = ops.guided_filter(g, planes, radius, eps).reshape(shape)
    return out if was_tensor else out.cpu().numpy()


def crf_labels(scores, guide, class_ids, th_factor, tau=0.1, **params):
    """The windowed CRF of include/asr_hip.h on the SR outputs of one image: ``scores`` [K, H, W] float32 (plane k: the SR output
    of class_ids[k]) and the colour ``guide`` [H, W, 3] (the RGB image at the score maps' size, values in [0, 1]) -> the int32
    label map [H, W]: ops.crf_refine of ops.crf_unaries(scores, th_factor, tau).  params: the fields of ops.check_crf (radius,
    dilation, iterations, w_app, w_smooth, theta_pos, theta_rgb, theta_smooth).  Runs on the device; returns a host array for
    host ``scores``, a device tensor otherwise."""
    was_tensor = isinstance(scores, torch.Tensor)
    p = ops.check_crf(params)
    tau = ops.check_crf_tau(tau)
    g = guide if isinstance(guide, torch.Tensor) else torch.as_tensor(np.asarray(guide, dtype=np.float32))
    if g.dim() != 3 or g.shape[2] != 3:
        raise ValueError(f"crf_labels: the guide must be [H, W, 3], got {tuple(g.shape)}")
    H, W = int(g.shape[0]), int(g.shape[1])
    ids = [int(c) for c in class_ids]
    s = scores if was_tensor else torch.as_tensor(np.asarray(scores, dtype=np.float32))
    if tuple(s.shape) != (len(ids), H, W):
        raise ValueError(f"crf_labels: scores must be [{len(ids)}, {H}, {W}], got {tuple(s.shape)}")
    dev = _lib.require_gpu()
    g = g.to(device=dev, dtype=torch.float32).contiguous()
    s = s.to(device=dev, dtype=torch.float32).contiguous()
    out = ops.crf_refine(g, ops.crf_unaries(s, th_factor, tau), ids, p)
    return out if was_tensor else out.cpu().numpy()


def threshold_sweep_IoU(true_image, image, class_id, th_factors, include_bg=False):
    """float64 [K]: the single-class IoU of ``image`` thresholded at each factor of ``th_factors`` (threshold_tests.py:113-121),
    i.e. ``[compute_IoU(true_image, threshold_image(image, class_id, th_factor=f), class_id=class_id, include_bg=include_bg)
    for f in th_factors]``, from one pass over the image for all factors (asr_threshold_sweep_iou_counts_f32)."""
    from ..utils import _as_label_tensor, iou_from_counts
    dev = _lib.require_gpu()
    img = image if isinstance(image, torch.Tensor) else torch.as_tensor(np.asarray(image, dtype=np.float32))
    img = img.to(device=dev, dtype=torch.float32).contiguous().reshape(1, -1)
    truth = _as_label_tensor(true_image, dev)
    if truth.numel() != img.numel():
        raise ValueError(f"expected {img.numel()} pixels in the label map, got {truth.numel()}")
    counts = ops.threshold_sweep_iou_counts(img, truth, th_factors, class_id, include_bg=include_bg).cpu().numpy()[0]
    return np.array([iou_from_counts(c, include_bg) for c in counts], dtype=np.float64)


# ---- interchange file (augmentation_utils.py:117-136 writer, superres_utils.py:154-210 reader) -------
def save_SR_data(path_without_ext, class_masks, max_masks, angles, shifts, filename, mode, angle_max, shift_max, ext=None):
    ext = ext or DATA_EXT
    os.makedirs(os.path.dirname(path_without_ext) or ".", exist_ok=True)
    data = dict(class_masks=np.asarray(class_masks, dtype=np.float32), angles=np.asarray(angles, dtype=np.float32),
                shifts=np.asarray(shifts, dtype=np.float32))
    if max_masks is not None and len(max_masks):
        data["max_masks"] = np.asarray(max_masks, dtype=np.float32)
    attrs = dict(filename=str(filename), mode=str(mode), angle_max=angle_max, shift_max=shift_max)
    if ext == ".npz":
        np.savez(path_without_ext + ext, **data, **{k: np.array(v) for k, v in attrs.items()})
    elif ext in (".hdf5", ".h5"):
        hdf5_lite.write(path_without_ext + ext, data, attrs)
    else:
        raise ValueError(f"unknown interchange format {ext!r} (.hdf5 or .npz)")
    return path_without_ext + ext


def _open_SR_file(filepath):
    """-> dict with the datasets plus the attributes 'filename' and 'mode' (either container format)."""
    if str(filepath).endswith(".npz"):
        with np.load(filepath, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    datasets, attrs = hdf5_lite.read(filepath)
    out = dict(datasets)
    out.update(attrs.get("/", {}))
    return out


def check_validity(file, num_aug=100):
    """Every array dataset has at least num_aug entries (superres_utils.py:108-115)."""
    for key in ("class_masks", "max_masks", "angles", "shifts"):
        if key in file and file[key].shape[0] < num_aug:
            return False
    return True


check_hdf5_validity = check_validity          # the reference's name (superres_utils.py:108)


def probe_SR_data(filepath, num_aug=100):
    """What load_SR_data WOULD do with this file, from its headers alone (no mask is read): (valid, solves) -- valid exactly
    when load_SR_data would not raise (readable, every array dataset with at least num_aug entries, name and mode present),
    solves = the Adam solves an evaluation of it runs (2 for slice_max files: class map and max map, else 1).  Used by the
    sharded evaluation loop, which must know both for EVERY file before its first solve (evaluation.py) and must not hold a
    shard's worth of masks in host memory to find out."""
    try:
        if str(filepath).endswith(".npz"):
            file = _open_SR_file(filepath)                      # (the .npz container has no cheap header; stage-1 default is .hdf5)
            shapes = {k: np.shape(v) for k, v in file.items()}
            mode = str(file["mode"])
            str(file["filename"])
        else:
            shapes, attrs = hdf5_lite.header(filepath)
            root = attrs.get("/", {})
            mode = str(root["mode"])
            str(root["filename"])
        for key in ("class_masks", "angles", "shifts") + (("max_masks",) if mode == "slice_max" else ()):
            if key not in shapes:
                return False, 0
        for key in ("class_masks", "max_masks", "angles", "shifts"):
            if key in shapes and (len(shapes[key]) == 0 or shapes[key][0] < num_aug):
                return False, 0
        return True, 2 if mode == "slice_max" else 1
    except Exception:
        return False, 0


def load_SR_data(filepath, num_aug=100, global_normalize=True):
    """Returns (class_masks [N,h,w,1], max_masks | None, angles, shifts, filename) as host arrays;
    argmax / slice_max masks are min-max normalised to [0,1] (superres_utils.py:183-206)."""
    file = _open_SR_file(filepath)
    if not check_validity(file, num_aug=num_aug):
        raise Exception(f"File: {filepath} is invalid")
    filename = str(file["filename"])
    mode = str(file["mode"])
    angles = file["angles"][:num_aug]
    shifts = file["shifts"][:num_aug]
    class_masks = file["class_masks"][:num_aug].astype(np.float32)
    max_masks = file["max_masks"][:num_aug].astype(np.float32) if mode == "slice_max" else None

    def normalise(stack):
        if global_normalize:
            gmin, gmax = stack.min(), stack.max()
            return np.stack([min_max_normalization(im, 0.0, 1.0, gmin, gmax) for im in stack]).astype(np.float32)
        return np.stack([min_max_normalization(im, 0.0, 1.0) for im in stack]).astype(np.float32)

    if mode != "slice":
        class_masks = normalise(class_masks)
    if max_masks is not None:
        max_masks = normalise(max_masks)
    return class_masks, max_masks, angles, shifts, filename


def _save_png(path, image, scale=True):
    from PIL import Image
    a = np.asarray(image, dtype=np.float32)
    a = a[..., 0] if a.ndim == 3 else a
    if scale:                                   # tf.keras.utils.save_img(scale=True)
        a = a - a.min()
        mx = a.max()
        if mx != 0:
            a = a / mx
        a = a * 255.0
    Image.fromarray(a.astype(np.uint8)).save(path)


SR_TYPES = ("aug", "mean", "max", "median", "trimmed_mean")      # compute_SR's SR_type ...
COVERED_SR_TYPES = ("covered_mean", "covered_median")             # ... and the coverage-normalised fusions it also accepts
EXTRA_SR_TYPES = ("median", "trimmed_mean") + COVERED_SR_TYPES    # the ones beyond the reference's three


def compute_SR(superresolution_obj, class_masks, angles, shifts, filename, dest_folder,
               SR_type="aug", max_masks=[], save_intermediate_output=False, save_final_output=False, class_id=8,
               th_factor=0.15, df_weights=None, tv_guide=None, guide=None, guide_radius=8, guide_eps=1e-3):
    """Dispatch aug / mean / max / median / trimmed_mean / covered_mean / covered_median SR, then threshold to a {0, class_id} mask [H,W,1] (host int32).
    guide ([H, W, 3] at the output size, the RGB image in [0, 1]): the target (and in slice_max the max map's target) goes
    through guided_refine(., guide, guide_radius, guide_eps) before it is thresholded and saved; None: nothing changes.
    tv_guide (the same kind of image; "aug" only) goes INTO the solve instead: the edge weights of its TV prior
    (Superresolution.augmented_superresolution(tv_guide=...)), for the class solve and the max map's.  The two are independent.
    df_weights (a device tensor [N, h, w]; "aug" only): the per-measurement weights of the solve's data term
    (Superresolution.augmented_superresolution(df_weights=...)), again for both solves; the loss itself is the object's df_loss."""
    if SR_type not in SR_TYPES + COVERED_SR_TYPES:
        raise ValueError("SR_type must be one of " + ", ".join(repr(t) for t in SR_TYPES + COVERED_SR_TYPES))
    if df_weights is not None and SR_type != "aug":
        raise ValueError(f"df_weights weight the data term of the iterative solve: SR_type must be 'aug', got {SR_type!r}")
    if tv_guide is not None and SR_type != "aug":
        raise ValueError(f"tv_guide weights the TV prior of the iterative solve: SR_type must be 'aug', got {SR_type!r}")
    out_folder = os.path.join(dest_folder, f"{SR_type}_SR")
    if not os.path.exists(out_folder):
        os.makedirs(out_folder)
    if SR_type == "aug":
        SR_function = superresolution_obj.augmented_superresolution
    elif SR_type == "mean":
        SR_function = superresolution_obj.mean_superresolution
    elif SR_type == "max":
        SR_function = superresolution_obj.max_superresolution
    elif SR_type == "median":
        SR_function = superresolution_obj.median_superresolution
    elif SR_type == "covered_mean":
        SR_function = superresolution_obj.covered_mean_superresolution
    elif SR_type == "covered_median":
        SR_function = superresolution_obj.covered_median_superresolution
    else:
        SR_function = superresolution_obj.trimmed_mean_superresolution

    extra = {k: v for k, v in (("tv_guide", tv_guide), ("df_weights", df_weights)) if v is not None}
    if extra:
        solve = SR_function
        SR_function = lambda copies, a, s: solve(copies, a, s, **extra)
    target_image_class, _ = SR_function(class_masks, angles, shifts)
    if guide is not None:
        target_image_class = guided_refine(target_image_class, guide, guide_radius, guide_eps)
    target_image_max = None
    # the max mask is super-resolved only when it was produced, i.e. in slice_max OPM
    if max_masks is not None and len(max_masks) == len(class_masks):
        target_image_max, _ = SR_function(max_masks, angles, shifts)
        if guide is not None:
            target_image_max = guided_refine(target_image_max, guide, guide_radius, guide_eps)
        th_mask = threshold_image(target_image_class, class_id, th_mask=target_image_max)
    else:
        th_mask = threshold_image(target_image_class, class_id, th_factor=th_factor)

    if save_intermediate_output:
        _save_png(f"{out_folder}/{filename}_class.png", target_image_class)
        if target_image_max is not None:
            _save_png(f"{out_folder}/{filename}_max.png", target_image_max)
    if save_final_output:
        _save_png(f"{out_folder}/{filename}_{SR_type}_SR.png", th_mask)
    return th_mask
