"""Prediction: class maps of images at the images' own size (or any other), from one trained network, the CPS pair as an
ensemble, and / or flipped test-time views.

The model forward gives low-resolution-or-not logits per view; ONE call of `nnf.resize_argmax` (vqseg_resize_argmax_f on the
GPU) undoes each view's flip, resizes bilinearly (align_corners=False, as evaluate.test_loop), averages the views' logits and
takes the arg-max -- the full-resolution (N, C, H, W) logit tensor of the scoring loop is never written.  Views are ordered
model-major, then in `tta` order; their number (models x tta) is 1, 2 or 4, so the mean's 1 / V is exact.

    Predictor(model, num_classes)(images).label                        # (N, H, W) uint8
    Predictor([m1, m2], 3, tta=("none", "hflip"))(images, size=(966, 1296), want_confidence=True)
"""
from collections import namedtuple
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple, Union

import torch
from torch import nn

from . import nnf

TTA_FLIPS = {"none": 0, "hflip": 1, "vflip": 2, "hvflip": 3}   # test-time view -> flip code of resize_argmax (bit 0 columns, bit 1 rows)

Prediction = namedtuple("Prediction", "label confidence")      # (N, H, W) uint8 class ids; (N, H, W) f32 top probability or None


class Predictor:
    """`models`: one nn.Module or a sequence (two: the CPS ensemble); `tta`: a selection of "none", "hflip", "vflip", "hvflip";
    len(models) * len(tta) must be 1, 2 or 4.  `amp_dtype`: the forwards run under torch.autocast on the GPU (None: fp32).
    `device`: where the images are moved to before the forward (None: they stay where they are)."""

    def __init__(self, models: Union[nn.Module, Sequence[nn.Module]], num_classes: int, amp_dtype=None, tta: Sequence[str] = ("none",),
                 device=None):
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

    def views(self, images: torch.Tensor):
        """-> (fp32 logits per view, flip code per view), model-major then tta order.  The models' modes are the caller's business."""
        if self.device is not None:
            images = images.to(self.device)
        logits, flips = [], []
        for model in self.models:
            for name in self.tta:
                code = TTA_FLIPS[name]
                x = images.flip(nnf.FLIP_DIMS[code]) if code else images          # an exact permutation: the un-flip is the same index map
                if self.amp_dtype is not None and x.is_cuda:
                    with torch.autocast("cuda", dtype=self.amp_dtype):
                        out = model(x)
                else:
                    out = model(x)
                out = out[0] if isinstance(out, tuple) else out
                if out.dim() != 4 or out.shape[1] != self.num_classes:
                    raise ValueError(f"the model returned logits of shape {tuple(out.shape)}, expected (N, {self.num_classes}, h, w)")
                logits.append(out.float())
                flips.append(code)
        return logits, flips

    @torch.no_grad()
    def __call__(self, images: torch.Tensor, size: Optional[Sequence[int]] = None, want_confidence: bool = False) -> Prediction:
        """images (N, 3, H, W) -> Prediction(label (N, Ho, Wo) uint8, confidence (N, Ho, Wo) f32 | None); size None: (H, W)."""
        size = tuple(images.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
        modes = [m.training for m in self.models]
        for m in self.models:
            m.eval()
        try:
            logits, flips = self.views(images)
            label, top, _ = nnf.resize_argmax(logits, size, flips=flips, want_top=want_confidence)
        finally:
            for m, was_training in zip(self.models, modes):
                m.train(was_training)
        return Prediction(label, top)

    @torch.no_grad()
    def render(self, images: torch.Tensor, targets: Optional[torch.Tensor] = None, size: Optional[Sequence[int]] = None, panels=None,
               half: bool = False, palette=None, alpha: float = 0.4) -> torch.Tensor:
        """images (N, 3, H, W) -> the panel sheet of their prediction, a uint8 (N * Ho, cols, 3) tensor (halved with `half`) on the
        images' device: the views of __call__ (ensemble and test-time views averaged inside nnf.resize_argmax), then one render
        launch (utils.visualize.render_sheet; vqseg_render_sheet_u8 on the GPU) from the labels, `targets` (N, Ht, Wt) at any size
        and the images themselves.  `panels` default: image | target | pred | 20 px white | mix_pred (without `targets`: no target
        panel); size None: (H, W)."""
        from .utils.visualize import GAP, render_sheet
        size = tuple(images.shape[-2:]) if size is None else (int(size[0]), int(size[1]))
        if panels is None:
            panels = ["image"] + (["target"] if targets is not None else []) + ["pred", ("fill", GAP), "mix_pred"]
        modes = [m.training for m in self.models]
        for m in self.models:
            m.eval()
        try:
            logits, flips = self.views(images)
        finally:
            for m, was_training in zip(self.models, modes):
                m.train(was_training)
        dev = logits[0].device
        return render_sheet(panels, images.to(dev), logits, None if targets is None else targets.to(dev), size=size, palette=palette, alpha=alpha,
                            half=half, flips=flips)

    def predict_batches(self, batches: Iterable, size: Optional[Sequence[int]] = None, want_confidence: bool = False) -> Iterator[Prediction]:
        """one Prediction per batch; a batch is the images or a tuple / list whose first entry they are ((images, labels), ...)"""
        for batch in batches:
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            yield self(images, size=size, want_confidence=want_confidence)


def predict_batches(models, batches: Iterable, num_classes: int, amp_dtype=None, tta: Sequence[str] = ("none",), device=None,
                    size: Optional[Sequence[int]] = None, want_confidence: bool = False) -> Iterator[Prediction]:
    """Predictor(models, num_classes, amp_dtype, tta, device).predict_batches(batches, size, want_confidence)"""
    return Predictor(models, num_classes, amp_dtype=amp_dtype, tta=tta, device=device).predict_batches(batches, size, want_confidence)
