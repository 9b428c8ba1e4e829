"""Evaluation loop (reference: test_detailviz.py:87-163 `test_loop`, without its wandb / visualisation side).

Eval-mode model (on the HIP path BatchNorm + residual + ReLU ride in the convolution epilogues, the VQ layers are pure
gathers), logits resized bilinearly to the native mask size, metrics per batch exactly as `Measurement.measure` defines
them (`measurement.py:7-91`: per-image confusion matrices, IoU with the +1e-8 denominator, batch means) and averaged
over the batches.  Only the (N, C, C) confusion counts and the per-image hit counts leave the device.

`fused=True` (opt-in) takes resize, arg-max and confusion counts of a batch from one `nnf.resize_argmax` call, so the logits at
mask size are never written; the per-image accuracy is then trace(counts) / (Hm * Wm) -- the same number as the mean of the
0 / 1 hits (an out-of-range target never equals a class, and a mean of 0 / 1 doubles is a ratio of integers), and the returned
dict equals the unfused one.  `tta` (with fused: "hflip", "vflip", "hvflip" beside "none") scores the mean over flipped views.

`visualize` (with fused) is a callable `(batch_index, viz_v1, viz_v2)` that receives, per batch, the two sheets test_detailviz.py:124-129
builds -- viz_v1 = [input | target | detailed prediction], viz_v2 = 0.6 input + 0.4 detailed prediction, at half the mask size, the
batch stacked vertically -- as uint8 numpy arrays: a second `nnf.resize_argmax` call at the display size and one render launch
(utils.visualize.render_sheet), after which only the sheet's bytes cross to the host.  The labels shown are the arg-max of the
network's logits resized directly to the display size (the reference resizes them to the mask size first, then again).  With None
nothing changes: no extra launch, the same dict.

`window` (with fused; `stride`, `blend`, `window_batch`, `net_size` as predict.Predictor takes them) scores tiled prediction: the
network runs on windows of the images and one `nnf.merge_argmax` call blends them and counts.  The images and masks of a batch must
then have the same size (e.g. BaseDataset(resize=None)); the sheets of `visualize` are not built for it.

`crf` (with fused; a utils.crf.DenseCRF or True for its defaults) scores the dense-CRF refinement of the prediction at the mask size,
as deprecated/test _crf.py does between the forward and the metrics: predict.Predictor(crf=...).refined, then the counts from one
`nnf.resize_argmax` call on the refined energies.  Not built with `window` or `visualize`.

`min_area` (with fused; `min_area_fill` a class id or "neighbour", `connectivity`, `region_ignore`) scores the area-filtered class maps of
predict.Predictor(min_area=...) in whatever mode is asked for: the counts come from the confusion kernel on the one-hot form of the filtered map.

`boundary` (with fused; True for the defaults or a dict of `tolerance`, `width`, `ignore` as utils.boundary.BoundaryMeasurement takes them)
adds contour-level scores of the label map the fused call of the branch returns anyway -- resize_argmax's, merge_argmax's or the Predictor's;
no second forward is made -- in every mode fused has: test_boundary_f1 / test_boundary_f1s, test_boundary_iou / test_boundary_ious (means
over all images, NaN skipped; the lists per class, rounded to 5 places) and test_hausdorff.  With None nothing changes: no extra launch, the
same dict.

`panoptic` (with fused; True for the defaults or a dict of `things`, `void`, `connectivity`, `capacity` as utils.instances.InstanceMeasurement
takes them) adds object-level scores of the same label map -- the area-filtered one when `min_area` is given; no second forward is made:
test_pq, test_sq, test_rq (panoptic quality = segmentation quality x recognition quality of the counts summed over all images; the means
over the thing classes) with test_pqs / test_sqs / test_rqs per class (rounded to 5 places, NaN for a class that is no thing),
test_count_error (the mean over images and thing classes of |regions predicted - regions in the ground truth|) and
test_panoptic_overflowed (the number of images with more regions than `capacity`, which are left out: raise it).  With None nothing changes.
"""
from typing import Dict, Iterable, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import nnf
from .measurement import BoundaryMeasurement, InstanceMeasurement, Measurement, confusion_matrix_device
from .predict import Predictor


def _resized_counts(model, img, target, num_classes, amp_dtype):
    """the two-step path: logits at mask size, then (N, C, C) confusion counts (rows = ground truth) and per-image accuracy"""
    if amp_dtype is not None and img.is_cuda:
        with torch.autocast("cuda", dtype=amp_dtype):
            pred = model(img)
    else:
        pred = model(img)
    pred = pred[0] if isinstance(pred, tuple) else pred
    pred = pred.float()
    # F.interpolate(pred, size, mode="bilinear") of test_detailviz.py:118 (align_corners=False): the HIP resize kernel on the device
    pred = nnf.upsample_bilinear(pred, size=tuple(target.shape[-2:]), align_corners=False) if pred.is_cuda else \
        F.interpolate(pred, target.shape[-2:], mode="bilinear")
    conf = confusion_matrix_device(pred, target, num_classes)                  # (N, C, C), rows = ground truth
    hits = (pred.argmax(dim=1) == target).flatten(1).double().mean(dim=1)       # Measurement.accuracy per image
    return conf, hits


def _detail_sheets(img, logits, flips, target, num_classes):
    """(viz_v1, viz_v2) of test_detailviz.py:124-129 for one batch, uint8 numpy: everything at half the mask size"""
    from .utils.visualize import default_palette, render_sheet
    size = (target.shape[-2] // 2, target.shape[-1] // 2)
    sheet = render_sheet(["image", "target", "detail", "mix_detail"], img, logits, target, size=size, palette=default_palette(num_classes),
                         flips=flips).cpu().numpy()
    return np.ascontiguousarray(sheet[:, :3 * size[1]]), np.ascontiguousarray(sheet[:, 3 * size[1]:])


@torch.no_grad()
def test_loop(model: torch.nn.Module, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], num_classes: int,
              device=None, amp_dtype=None, fused: bool = False, tta=None, visualize=None, window=None, stride=None,
              blend: str = "linear", window_batch=None, net_size=None, crf=None, min_area=None, min_area_fill=0, connectivity: int = 4,
              region_ignore=(), boundary=None, panoptic=None) -> Dict[str, object]:
    """batches yields (images (N, 3, H, W) float in [0, 1], labels (N, Hm, Wm) int class ids)."""
    if panoptic is not None and not fused:
        raise ValueError("test_loop: panoptic needs fused=True (the regions are those of the fused path's class maps)")
    if panoptic is not None and panoptic is not True and not (isinstance(panoptic, dict) and set(panoptic) <= {"things", "void", "connectivity", "capacity"}):
        raise ValueError(f"test_loop: panoptic is None, True or a dict of things, void, connectivity and capacity, got {panoptic!r}")
    objects = None if panoptic is None else InstanceMeasurement(num_classes, **({} if panoptic is True else panoptic))
    if boundary is not None and not fused:
        raise ValueError("test_loop: boundary needs fused=True (the contours are those of the fused path's class maps)")
    if boundary is not None and boundary is not True and not (isinstance(boundary, dict) and set(boundary) <= {"tolerance", "width", "ignore"}):
        raise ValueError(f"test_loop: boundary is None, True or a dict of tolerance, width and ignore, got {boundary!r}")
    contours = None if boundary is None else BoundaryMeasurement(num_classes, **({} if boundary is True else boundary))
    if min_area is not None and not fused:
        raise ValueError("test_loop: min_area needs fused=True (the filter runs on the fused path's class maps)")
    if min_area is not None and visualize is not None:
        raise ValueError("test_loop: visualize is not built for the scoring of area-filtered maps (min_area=...)")
    if min_area is not None and (isinstance(min_area_fill, bool) or not (min_area_fill == "neighbour" or (
            isinstance(min_area_fill, int) and 0 <= min_area_fill < num_classes))):
        raise ValueError(f"test_loop: a scored map holds classes only: min_area_fill must be a class id or 'neighbour', got {min_area_fill!r}")
    if window is not None and not fused:
        raise ValueError("test_loop: window needs fused=True (the windows are blended inside the fused merge + arg-max)")
    if window is not None and visualize is not None:
        raise ValueError("test_loop: visualize is not built for tiled scoring (window=...)")
    if tta is not None and not fused:
        raise ValueError("test_loop: tta needs fused=True (the views are averaged inside the fused resize + arg-max)")
    if visualize is not None and not fused:
        raise ValueError("test_loop: visualize needs fused=True (the sheets are drawn from the fused path's views)")
    if crf is not None and not fused:
        raise ValueError("test_loop: crf needs fused=True (the refined energies are scored by the fused arg-max + counts)")
    if crf is not None and visualize is not None:
        raise ValueError("test_loop: visualize is not built for CRF scoring (crf=...)")
    predictor = Predictor(model, num_classes, amp_dtype=amp_dtype, tta=tta or ("none",), window=window, stride=stride, blend=blend,
                          window_batch=window_batch, net_size=net_size, crf=crf, min_area=min_area, min_area_fill=min_area_fill,
                          connectivity=connectivity, region_ignore=region_ignore) if fused else None
    views = predictor.views if fused else None
    was_training = model.training
    model.eval()
    meas = Measurement(num_classes)
    sums = dict(test_acc=0.0, test_miou=0.0, test_precision=0.0, test_recall=0.0, test_f1score=0.0)
    iou_per_class = np.zeros(num_classes, dtype=np.float64)
    n_batches = 0
    try:
        for img, target in batches:
            if device is not None:
                img, target = img.to(device), target.to(device)
            if fused and min_area is not None:
                # the filtered class map of predict.Predictor in whatever mode, counted by the confusion kernel from its one-hot form
                size = tuple(target.shape[-2:])
                label = predictor(img, size=None if window is not None else size).label
                if tuple(label.shape[-2:]) != size:
                    raise ValueError(f"test_loop: tiled scoring needs images and masks of one size, got {tuple(label.shape[-2:])} and {size}")
                onehot = (label[:, None] == torch.arange(num_classes, device=label.device, dtype=label.dtype)[None, :, None, None]).float()
                conf = confusion_matrix_device(onehot, target.to(label.device), num_classes)
                hits = torch.diagonal(conf, dim1=1, dim2=2).sum(dim=1).double() / (size[0] * size[1])
            elif fused and window is not None:
                if tuple(img.shape[-2:]) != tuple(target.shape[-2:]):
                    raise ValueError(f"test_loop: tiled scoring needs images and masks of one size, got {tuple(img.shape[-2:])} and "
                                     f"{tuple(target.shape[-2:])} (e.g. BaseDataset(resize=None))")
                logits, flips, grid = predictor.tiled_views(img)
                label, _top, conf = nnf.merge_argmax(logits, grid, flips=flips, blend=blend, target=target)
                hits = torch.diagonal(conf, dim1=1, dim2=2).sum(dim=1).double() / (target.shape[-2] * target.shape[-1])
            elif fused and predictor.crf is not None:
                size = tuple(target.shape[-2:])
                label, _top, conf = nnf.resize_argmax(predictor.refined(img, size), size, target=target)
                hits = torch.diagonal(conf, dim1=1, dim2=2).sum(dim=1).double() / (size[0] * size[1])
            elif fused:
                logits, flips = views(img)
                label, _top, conf = nnf.resize_argmax(logits, tuple(target.shape[-2:]), flips=flips, target=target)
                hits = torch.diagonal(conf, dim1=1, dim2=2).sum(dim=1).double() / (target.shape[-2] * target.shape[-1])
                if visualize is not None:
                    visualize(n_batches, *_detail_sheets(img, logits, flips, target, num_classes))
            else:
                conf, hits = _resized_counts(model, img, target, num_classes, amp_dtype)
            if contours is not None:
                contours.update(label, target.to(label.device))
            if objects is not None:
                objects.update(label, target.to(label.device))
            conf_np = conf.cpu().numpy()
            miou, ious = meas.miou(conf_np)
            precision, _ = meas.precision(conf_np)
            recall, _ = meas.recall(conf_np)
            sums["test_acc"] += float(hits.mean())
            sums["test_miou"] += float(miou)
            sums["test_precision"] += float(precision)
            sums["test_recall"] += float(recall)
            sums["test_f1score"] += float(meas.f1score(recall, precision))
            iou_per_class += np.array(ious)
            n_batches += 1
    finally:                                                 # whatever ends the loop, a refusal included
        model.train(was_training)
    if n_batches == 0:
        raise ValueError("test_loop: no batches")
    out = {k: v / n_batches for k, v in sums.items()}
    out["test_ious"] = np.round(iou_per_class / n_batches, 5).tolist()
    if contours is not None:
        r = contours.result()
        out["test_boundary_f1"], out["test_boundary_f1s"] = r["boundary_f1"], np.round(r["boundary_f1s"], 5).tolist()
        out["test_boundary_iou"], out["test_boundary_ious"] = r["boundary_iou"], np.round(r["boundary_ious"], 5).tolist()
        out["test_hausdorff"] = r["hausdorff"]
    if objects is not None:
        r = objects.result()
        for key in ("pq", "sq", "rq"):
            out["test_" + key], out["test_" + key + "s"] = r[key], np.round(r[key + "s"], 5).tolist()
        out["test_count_error"], out["test_panoptic_overflowed"] = r["count_error"], r["overflowed"]
    return out
