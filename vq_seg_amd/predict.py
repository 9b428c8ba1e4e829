"""Prediction: class maps of images at the images' own size (or any other), from one trained network, the CPS pair as an
ensemble, and / or flipped test-time views.

The model forward gives low-resolution-or-not logits per view; ONE call of `nnf.resize_argmax` (vqseg_resize_argmax_f on the
GPU) undoes each view's flip, resizes bilinearly (align_corners=False, as evaluate.test_loop), averages the views' logits and
takes the arg-max -- the full-resolution (N, C, H, W) logit tensor of the scoring loop is never written.  Views are ordered
model-major, then in `tta` order; their number (models x tta) is 1, 2 or 4, so the mean's 1 / V is exact.

    Predictor(model, num_classes)(images).label                        # (N, H, W) uint8
    Predictor([m1, m2], 3, tta=("none", "hflip"))(images, size=(966, 1296), want_confidence=True)

Tiled (sliding-window) prediction, `window=...`: the network runs on native-resolution windows of the images instead of the whole
image squeezed to its training size, and overlapping windows are blended with a weight that falls off towards each window's border.
ONE `nnf.extract_windows` launch (vqseg_extract_windows_f) cuts, resizes and flips the windows of all test-time views, the forwards
run over them in chunks of `window_batch`, and ONE `nnf.merge_argmax` launch (vqseg_merge_argmax_f) blends the windows, averages the
views and takes the arg-max -- again without a full-resolution logit tensor.  The window grid is nnf.window_starts' (the last window
of an axis is clamped to end at the border).  Not built: windows larger than the image (padding), rotated views, averaging
probabilities instead of logits.

    Predictor(model, 3, window=512)(images).label                      # stride 256, "linear" blend, at the images' own size
    Predictor([m1, m2], 3, tta=("none", "hflip"), window=(512, 640), stride=384, window_batch=8)(images, want_confidence=True)

Dense-CRF refinement, `crf=...` (a utils.crf.DenseCRF, or True for the reference's defaults; untiled mode only): the views' logits are
resized to `size` (nnf.upsample_bilinear, align_corners=False), un-flipped, averaged and passed through softmax; the images are
resized the same way if `size` is not their own; `nnf.dense_crf(out="logits")` refines the probabilities under the images
(vqseg_crf_prepare_f, vqseg_crf_step_f) and `nnf.resize_argmax` at equal size takes labels, top probability and counts from the
refined energies.  Not built: the CRF under tiled prediction, and the reference script's order "CRF at the network's size, then
resize Q" -- which `size=` equal to the network's gives.

    Predictor(model, 3, crf=True)(images).label
    Predictor(model, 3, crf=DenseCRF(iter_max=5, truncate=None))(images, size=(966, 1296), want_confidence=True)

Regions, `min_area=...` (every mode): after the arg-max, connected regions of one class (utils.regions; vqseg_region_* on the GPU) with
fewer than `min_area` pixels are replaced -- by `min_area_fill`, a class id or "neighbour" -- so specks of predicted weed and pinholes
in a plant go.  `Predictor.instances` returns the prediction together with the table of its regions: the plants, with class, area,
bounding box and centroid.  Under tiled prediction the filter runs on the merged map.

    Predictor(model, 3, min_area=64, min_area_fill="neighbour")(images).label
    pred, plants = Predictor(model, 3, min_area=64).instances(images, classes=(1, 2))       # plants.count, .value, .area, .bbox, .centroid
"""
from collections import namedtuple
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import torch
from torch import nn

from . import nnf

TTA_FLIPS = {"none": 0, "hflip": 1, "vflip": 2, "hvflip": 3}   # test-time view -> flip code of resize_argmax (bit 0 columns, bit 1 rows)

Prediction = namedtuple("Prediction", "label confidence")      # (N, H, W) uint8 class ids; (N, H, W) f32 top probability or None


def _as_crf(crf):
    """None, a utils.crf.DenseCRF, or True for one with the reference's defaults"""
    from .utils.crf import DenseCRF
    if crf is None or crf is False:
        return None
    if crf is True:
        return DenseCRF()
    if not isinstance(crf, DenseCRF):
        raise TypeError(f"crf must be a utils.crf.DenseCRF, True or None, got {type(crf).__name__}")
    return crf


def _as_superpixels(superpixels):
    """None, a component count, or dict(num_components=, compactness=, iters=) -> None or the full dict"""
    if superpixels is None:
        return None
    given = dict(superpixels) if isinstance(superpixels, dict) else dict(num_components=superpixels)
    unknown = sorted(set(given) - {"num_components", "compactness", "iters"})
    if unknown or "num_components" not in given:
        raise ValueError(f"superpixels is a component count or dict(num_components=, compactness=, iters=), got {superpixels!r}")
    k, m, iters = given["num_components"], given.get("compactness", 10.0), given.get("iters", 10)
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"superpixels: num_components must be a positive integer, got {k!r}")
    if not 0.0 <= float(m) <= 1e9:
        raise ValueError(f"superpixels: compactness must lie in [0, 1e9], got {m!r}")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"superpixels: iters must be an integer >= 0, got {iters!r}")
    return dict(num_components=k, compactness=float(m), iters=iters)


def _resize(x: torch.Tensor, size) -> torch.Tensor:
    """bilinear, align_corners=False: the HIP resize kernel on the GPU, F.interpolate elsewhere"""
    if x.is_cuda:
        return nnf.upsample_bilinear(x, size=tuple(size), align_corners=False)
    return torch.nn.functional.interpolate(x, tuple(size), mode="bilinear", align_corners=False)


class Predictor:
    """`models`: one nn.Module or a sequence (two: the CPS ensemble); `tta`: a selection of "none", "hflip", "vflip", "hvflip";
    len(models) * len(tta) must be 1, 2 or 4.  `amp_dtype`: the forwards run under torch.autocast on the GPU (None: fp32).
    `device`: where the images are moved to before the forward (None: they stay where they are).
    `window` (an int or (h, w) in image pixels; None: the whole image goes through the network, as above) turns tiled prediction on:
    `stride` (default window // 2), `blend` ("linear" or "uniform": nnf.merge_argmax), `net_size` (what the network sees of a
    window, if not the window itself: the windows are resized bilinearly on the way in and their logits on the way out) and
    `window_batch` (how many windows go through one forward, default all of a view: it bounds the forward's activations).  The
    logits of ALL windows are held until the merge: B * T * C * lh * lw * 4 bytes per view (B images, T windows each, C classes,
    lh x lw logits per window).  `crf`: a utils.crf.DenseCRF, or True for its defaults, refines the prediction (untiled mode).
    `superpixels`: a component count K or dict(num_components=, compactness=, iters=) -- object-based smoothing, the cheap alternative
    to the CRF (the reference's users write pred[assignment]): the view-averaged class probabilities are averaged over SLIC
    superpixels of the images (utils.superpixel) at the network's size, between the softmax and the arg-max.  Inference only; not
    with `window` or `crf`.
    `min_area` (None: off, nothing is launched): in every mode the class map is filtered after the arg-max -- a connected region
    (`connectivity` 4 or 8) of one class with fewer than `min_area` pixels takes `min_area_fill`, a class id (default 0, the
    background) or "neighbour" (utils.regions.remove_small_regions); pixels of a class in `region_ignore` belong to no region and stay.
    `confidence` stays the network's top probability at every pixel, also where the filter changed the class."""

    def __init__(self, models: Union[nn.Module, Sequence[nn.Module]], num_classes: int, amp_dtype=None, tta: Sequence[str] = ("none",),
                 device=None, window=None, stride=None, blend: str = "linear", window_batch: Optional[int] = None, net_size=None, crf=None,
                 superpixels=None, min_area: Optional[int] = None, min_area_fill=0, connectivity: int = 4, region_ignore=()):
        self.models: List[nn.Module] = [models] if isinstance(models, nn.Module) else list(models)
        self.tta: Tuple[str, ...] = (tta,) if isinstance(tta, str) else tuple(tta)
        unknown = [t for t in self.tta if t not in TTA_FLIPS]
        if unknown:
            raise ValueError(f"tta views are {sorted(TTA_FLIPS)}, got {unknown}")
        if not all(isinstance(m, nn.Module) for m in self.models):
            raise TypeError("models must be an nn.Module or a sequence of them")
        n_views = len(self.models) * len(self.tta)
        if n_views not in (1, 2, 4):
            raise ValueError(f"len(models) * len(tta) must be 1, 2 or 4 (the mean over the views is an exact scale), got "
                             f"{len(self.models)} x {len(self.tta)} = {n_views}")
        if not 2 <= int(num_classes) <= 4:
            raise ValueError(f"num_classes must be 2..4, got {num_classes}")
        self.num_classes, self.amp_dtype, self.device = int(num_classes), amp_dtype, device
        if window is None and (stride is not None or window_batch is not None or net_size is not None):
            raise ValueError("stride, window_batch and net_size belong to tiled prediction: give a window")
        if blend not in nnf.BLENDS:
            raise ValueError(f"blend is one of {sorted(nnf.BLENDS)}, got {blend!r}")
        if window_batch is not None and int(window_batch) < 1:
            raise ValueError(f"window_batch must be positive, got {window_batch}")
        self.window, self.stride, self.blend, self.net_size = window, stride, blend, net_size
        self.window_batch = None if window_batch is None else int(window_batch)
        self.crf = _as_crf(crf)
        if self.crf is not None and window is not None:
            raise ValueError("crf together with window: the CRF under tiled prediction is not built")
        self.superpixels = _as_superpixels(superpixels)
        if self.superpixels is not None and window is not None:
            raise ValueError("superpixels together with window: superpixels under tiled prediction are not built")
        if self.superpixels is not None and self.crf is not None:
            raise ValueError("superpixels together with crf: one refinement of the probabilities at a time")
        self.connectivity, self.region_ignore = nnf.region_settings(connectivity, region_ignore, "Predictor")
        self.min_area = None if min_area is None else nnf.region_min_area(min_area, "Predictor")
        nnf.region_fill(min_area_fill, torch.uint8, "Predictor: min_area_fill")
        self.min_area_fill = min_area_fill

    def _filtered(self, label: torch.Tensor) -> torch.Tensor:
        """the class map after the area filter (min_area None: the map itself, nothing is launched)"""
        if self.min_area is None:
            return label
        from .utils.regions import remove_small_regions
        return remove_small_regions(label, self.min_area, self.connectivity, self.region_ignore, fill=self.min_area_fill)

    def _forward(self, model: nn.Module, x: torch.Tensor) -> torch.Tensor:
        """fp32 logits of one forward, under autocast on the GPU if asked for"""
        if self.amp_dtype is not None and x.is_cuda:
            with torch.autocast("cuda", dtype=self.amp_dtype):
                out = model(x)
        else:
            out = model(x)
        out = out[0] if isinstance(out, tuple) else out
        if out.dim() != 4 or out.shape[1] != self.num_classes:
            raise ValueError(f"the model returned logits of shape {tuple(out.shape)}, expected (N, {self.num_classes}, h, w)")
        return out.float()

    def tiled_views(self, images: torch.Tensor):
        """tiled mode -> (fp32 window logits (B * T, C, lh, lw) per view, flip code per view, the nnf.WindowGrid): one extract launch
        for the flips of all views, then the forwards in chunks of `window_batch` per model x flip.  Views are ordered as `views`
        orders them.  The models' modes are the caller's business."""
        if self.window is None:
            raise ValueError("tiled_views: this Predictor has no window")
        if self.device is not None:
            images = images.to(self.device)
        if images.dim() != 4:
            raise ValueError(f"images must be (N, 3, H, W), got {tuple(images.shape)}")
        wh, ww = (int(self.window),) * 2 if isinstance(self.window, int) else (int(self.window[0]), int(self.window[1]))
        if wh > images.shape[-2] or ww > images.shape[-1]:
            raise ValueError(f"a window of {(wh, ww)} is larger than the images of {tuple(images.shape[-2:])}: padding is not built")
        codes = [TTA_FLIPS[name] for name in self.tta]
        windows, grid = nnf.extract_windows(images.float(), (wh, ww), self.stride, self.net_size, flips=codes)
        rows = windows.shape[1]
        step = rows if self.window_batch is None else self.window_batch
        logits, flips = [], []
        for model in self.models:
            for k, code in enumerate(codes):
                outs = [self._forward(model, windows[k, at:at + step]) for at in range(0, rows, step)]
                logits.append(outs[0] if len(outs) == 1 else torch.cat(outs))
                flips.append(code)
        return logits, flips, grid

    def _own_size(self, images: torch.Tensor, size) -> Tuple[int, int]:
        """tiled mode predicts at the images' own size only"""
        own = tuple(int(n) for n in images.shape[-2:])
        if size is not None and (int(size[0]), int(size[1])) != own:
            raise ValueError(f"tiled prediction is at the images' own size {own}, got size {tuple(size)}")
        return own

    def views(self, images: torch.Tensor):
        """-> (fp32 logits per view, flip code per view), model-major then tta order.  The models' modes are the caller's business."""
        if self.device is not None:
            images = images.to(self.device)
        logits, flips = [], []
        for model in self.models:
            for name in self.tta:
                code = TTA_FLIPS[name]
                x = images.flip(nnf.FLIP_DIMS[code]) if code else images          # an exact permutation: the un-flip is the same index map
                logits.append(self._forward(model, x))
                flips.append(code)
        return logits, flips

    def refined(self, images: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
        """crf mode -> the refined energies (N, C, Ho, Wo) fp32 at `size`: softmax of the views' mean logits there, then the dense
        CRF under the images brought to the same size.  The models' modes are the caller's business."""
        if self.crf is None:
            raise ValueError("refined: this Predictor has no crf")
        if self.device is not None:
            images = images.to(self.device)
        logits, flips = self.views(images)
        acc = None
        for v, code in zip(logits, flips):
            r = v if tuple(v.shape[-2:]) == tuple(size) else _resize(v, size)
            r = r.flip(nnf.FLIP_DIMS[code]) if code else r
            acc = r if acc is None else acc + r
        if len(logits) > 1:
            acc = acc * (1.0 / len(logits))
        x = images.to(acc.device).float()
        if tuple(x.shape[-2:]) != tuple(size):
            x = _resize(x, size)
        return self.crf.batch(x, torch.softmax(acc, dim=1), out="logits")

    def probabilities(self, images: torch.Tensor) -> torch.Tensor:
        """-> the class probabilities (N, C, h, w) fp32 at the network's size: softmax of the mean of the views' logits (each view
        un-flipped).  The models' modes are the caller's business."""
        logits, flips = self.views(images)
        acc = None
        for v, code in zip(logits, flips):
            r = v.flip(nnf.FLIP_DIMS[code]) if code else v
            acc = r if acc is None else acc + r
        if len(logits) > 1:
            acc = acc * (1.0 / len(logits))
        return torch.softmax(acc, dim=1)

    def pooled(self, images: torch.Tensor) -> torch.Tensor:
        """superpixels mode -> log of the pooled probabilities (N, C, h, w) fp32 at the network's size (softmax of it IS the pooled
        probabilities, so resize_argmax takes labels and top probability from it): `probabilities`, averaged over the SLIC superpixels
        of the images at that size."""
        from .utils.superpixel import slic, superpixel_mean
        if self.superpixels is None:
            raise ValueError("pooled: this Predictor has no superpixels")
        if self.device is not None:
            images = images.to(self.device)
        prob = self.probabilities(images)
        x = images.to(prob.device).float()
        if tuple(x.shape[-2:]) != tuple(prob.shape[-2:]):
            x = _resize(x, prob.shape[-2:])
        labels, _centers, (gy, gx) = slic(x, return_centers=True, **self.superpixels)
        return superpixel_mean(prob, labels, gy * gx).clamp_min(1e-30).log()

    @torch.no_grad()
    def __call__(self, images: torch.Tensor, size: Optional[Sequence[int]] = None, want_confidence: bool = False) -> Prediction:
        """images (N, 3, H, W) -> Prediction(label (N, Ho, Wo) uint8, confidence (N, Ho, Wo) f32 | None); size None: (H, W).
        Tiled mode: `size` must be None or the images' own."""
        size = self._own_size(images, size) if self.window is not None else \
            tuple(images.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
        modes = [m.training for m in self.models]
        for m in self.models:
            m.eval()
        try:
            if self.window is not None:
                logits, flips, grid = self.tiled_views(images)
                label, top, _ = nnf.merge_argmax(logits, grid, flips=flips, blend=self.blend, want_top=want_confidence)
            elif self.crf is not None:
                label, top, _ = nnf.resize_argmax(self.refined(images, size), size, want_top=want_confidence)
            elif self.superpixels is not None:
                label, top, _ = nnf.resize_argmax(self.pooled(images), size, want_top=want_confidence)
            else:
                logits, flips = self.views(images)
                label, top, _ = nnf.resize_argmax(logits, size, flips=flips, want_top=want_confidence)
        finally:
            for m, was_training in zip(self.models, modes):
                m.train(was_training)
        return Prediction(self._filtered(label), top)

    @torch.no_grad()
    def instances(self, images: torch.Tensor, size: Optional[Sequence[int]] = None, classes: Optional[Sequence[int]] = None,
                  capacity: int = 1024, want_confidence: bool = False):
        """images -> (Prediction, utils.regions.Regions): the prediction of __call__ (filtered, with `min_area`) and the table of its
        connected regions per image -- count, and per region its class (`value`), area, bounding box, centroid and first pixel;
        `capacity` rows per image.  `classes`: the class ids that count (e.g. (1, 2): crop and weed, not the background); pixels of
        any other class, and of a value in `region_ignore`, belong to no region.  None: every value outside `region_ignore`.  (At most
        four values can be ignored; with num_classes <= 4 only a `region_ignore` of values that are no class ids can exceed that.)"""
        from .utils.regions import region_table
        ignore = set(self.region_ignore)
        if classes is not None:
            wanted = set()
            for c in classes:
                if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < self.num_classes:
                    raise ValueError(f"instances: classes are ids in 0..{self.num_classes - 1}, got {tuple(classes)!r}")
                wanted.add(int(c))
            ignore |= set(range(self.num_classes)) - wanted
        if len(ignore) > 4:
            raise ValueError(f"instances: at most 4 values can be ignored, got {sorted(ignore)}")
        pred = self(images, size=size, want_confidence=want_confidence)
        return pred, region_table(pred.label, self.connectivity, tuple(sorted(ignore)), capacity)

    @torch.no_grad()
    def render(self, images: torch.Tensor, targets: Optional[torch.Tensor] = None, size: Optional[Sequence[int]] = None, panels=None,
               half: bool = False, palette=None, alpha: float = 0.4) -> torch.Tensor:
        """images (N, 3, H, W) -> the panel sheet of their prediction, a uint8 (N * Ho, cols, 3) tensor (halved with `half`) on the
        images' device: the views of __call__ (ensemble and test-time views averaged inside nnf.resize_argmax), then one render
        launch (utils.visualize.render_sheet; vqseg_render_sheet_u8 on the GPU) from the labels, `targets` (N, Ht, Wt) at any size
        and the images themselves.  `panels` default: image | target | pred | 20 px white | mix_pred (without `targets`: no target
        panel); size None: (H, W).  Tiled mode: the merged labels of __call__ are what the sheet shows (`size`: None or the
        images' own).  crf and superpixels mode: likewise the refined labels of __call__.  With `min_area` the sheet shows the
        filtered labels in every mode (the plain mode then takes the label path too)."""
        from .utils.visualize import GAP, render_sheet
        size = self._own_size(images, size) if self.window is not None else \
            tuple(images.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
        if panels is None:
            panels = ["image"] + (["target"] if targets is not None else []) + ["pred", ("fill", GAP), "mix_pred"]
        modes = [m.training for m in self.models]
        for m in self.models:
            m.eval()
        try:
            if self.window is not None:
                logits, flips, grid = self.tiled_views(images)
                label = nnf.merge_argmax(logits, grid, flips=flips, blend=self.blend)[0]
            elif self.crf is not None or self.superpixels is not None:
                logits = [self.refined(images, size) if self.crf is not None else self.pooled(images)]
                label = nnf.resize_argmax(logits, size)[0]
            else:
                logits, flips = self.views(images)
                if self.min_area is not None:
                    label = nnf.resize_argmax(logits, size, flips=flips)[0]
        finally:
            for m, was_training in zip(self.models, modes):
                m.train(was_training)
        dev = logits[0].device
        if self.window is not None or self.crf is not None or self.superpixels is not None or self.min_area is not None:
            return render_sheet(panels, images.to(dev), self._filtered(label), None if targets is None else targets.to(dev), size=size, palette=palette,
                                alpha=alpha, half=half, num_classes=self.num_classes)
        return render_sheet(panels, images.to(dev), logits, None if targets is None else targets.to(dev), size=size, palette=palette, alpha=alpha,
                            half=half, flips=flips)

    def predict_batches(self, batches: Iterable, size: Optional[Sequence[int]] = None, want_confidence: bool = False) -> Iterator[Prediction]:
        """one Prediction per batch; a batch is the images or a tuple / list whose first entry they are ((images, labels), ...)"""
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            yield self(images, size=size, want_confidence=want_confidence)


def predict_batches(models, batches: Iterable, num_classes: int, amp_dtype=None, tta: Sequence[str] = ("none",), device=None,
                    size: Optional[Sequence[int]] = None, want_confidence: bool = False, window=None, stride=None, blend: str = "linear",
                    window_batch: Optional[int] = None, net_size=None, crf=None, min_area: Optional[int] = None, min_area_fill=0,
                    connectivity: int = 4, region_ignore=()) -> Iterator[Prediction]:
    """Predictor(models, num_classes, amp_dtype, tta, device, window, stride, blend, window_batch, net_size, crf, min_area=...)
    .predict_batches(batches, size, want_confidence)"""
    return Predictor(models, num_classes, amp_dtype=amp_dtype, tta=tta, device=device, window=window, stride=stride, blend=blend,
                     window_batch=window_batch, net_size=net_size, crf=crf, min_area=min_area, min_area_fill=min_area_fill,
                     connectivity=connectivity, region_ignore=region_ignore).predict_batches(batches, size, want_confidence)
