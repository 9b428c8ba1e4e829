"""CutMix / CutOut (reference: data/augmentations.py:11-104; registered in data/__init__.py:1-7; driven by
deprecated/train_vqpt_easyhard_aug.py:90,119-123).  The strong-augmentation half of cross pseudo supervision: the unlabelled
training forwards see box-mixed images, and the pseudo targets are mixed with the same box.

The box draw is the reference's, draw for draw (`draw_box`), so a seeded run of the reference's augmentation code and of this one
pick the same boxes.  CPU tensors take the reference's arithmetic (batch * mask + partner * (1 - mask)) with torch ops; tensors on
the GPU take ONE HIP pass per tensor (`_hip.box_mix`, vqseg_box_mix_f) that selects by bits.  The two agree on every finite value
(0 / 1 masks make the arithmetic a selection); they differ only where arithmetic is not a selection: the reference turns -0.0 into
+0.0 and spreads a NaN / inf of the partner over the whole image (x * 1 + nan * 0), the kernel passes every bit pattern through.

Not built: similarity_transform / inverse_similarity_transform (data/augmentations.py:108-148; their rotations discard their result).
"""
from __future__ import annotations

import random
import weakref
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _hip

Box = Tuple[int, int, int, int]                 # (y1, x1, cut_h, cut_w): rows [y1, y1 + cut_h), columns [x1, x1 + cut_w)


def _dense(t: torch.Tensor) -> torch.Tensor:
    """the two layouts the kernel walks: contiguous or channels_last (anything else is copied once)"""
    return t if (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))) else t.contiguous()


def _np_randint(rng, low: int, high: int) -> int:
    """an integer of [low, high) from np.random / a RandomState (`randint`) or a Generator (`integers`)"""
    return int(rng.randint(low, high) if hasattr(rng, "randint") else rng.integers(low, high))


def draw_box(h: int, w: int, ratio: float, np_rng=None, py_rng=None) -> Box:
    """The box of make_cutout_mask / CutMix._make_mask (data/augmentations.py:32-39, 53-60), same draws in the same order:
        cut_w = np.random.randint(int(w * ratio) + 1, w);  cut_h = int(h * w * ratio // cut_w)
        x1 = np.random.randint(0, w - cut_w + 1);          y1 = random.randint(0, h - cut_h + 1)
    `y1` comes from PYTHON's generator, whose upper bound is inclusive: y1 may be h - cut_h + 1, one row too low, and the reference's
    slice mask[y1:y1 + cut_h] then silently loses the box's last row.  That quirk is kept: the box returned is the box the reference's
    mask shows, i.e. clipped to the image (so y1 + cut_h <= h always holds here, and cut_h may come back one smaller than drawn).
    `np_rng` (np.random, a RandomState or a Generator) and `py_rng` (random or a random.Random) default to the GLOBAL generators,
    which is what the reference consumes."""
    h, w = int(h), int(w)
    if h <= 0 or w <= 0:
        raise ValueError(f"draw_box: image size must be positive, got {h} x {w}")
    if not 0.0 <= ratio < 1.0:
        raise ValueError(f"draw_box: ratio must lie in [0, 1), got {ratio}")
    if int(w * ratio) + 1 >= w:
        raise ValueError(f"draw_box: ratio {ratio} leaves no box width to draw for w = {w}: int(w * ratio) + 1 = {int(w * ratio) + 1} must be "
                         f"below w (the reference's np.random.randint(low, high) raises for low >= high)")
    np_rng = np.random if np_rng is None else np_rng
    py_rng = random if py_rng is None else py_rng
    cut_w = _np_randint(np_rng, int(w * ratio) + 1, w)
    cut_h = int(h * w * ratio // cut_w)
    x1 = _np_randint(np_rng, 0, w - cut_w + 1)
    y1 = int(py_rng.randint(0, h - cut_h + 1))              # inclusive upper bound (see above)
    y1 = min(y1, h)
    return y1, x1, min(cut_h, h - y1), cut_w


def box_mask(img_size: Iterable[int], box: Box) -> torch.Tensor:
    """(H, W) int64: ones, zeros in the box"""
    y1, x1, ch, cw = box
    mask = torch.ones(tuple(img_size), dtype=torch.int64)
    mask[y1:y1 + ch, x1:x1 + cw] = 0
    return mask


def make_cutout_mask(img_size: Iterable[int], ratio: float) -> torch.Tensor:
    """data/augmentations.py:32-39 (global generators)"""
    img_size = tuple(img_size)
    return box_mask(img_size, draw_box(img_size[0], img_size[1], ratio))


def step_generators(seed: int, rank: int, it: int):
    """(np_rng, py_rng) for draw_box as a pure function of (seed, rank, iteration): what CPSTrainer draws its boxes from.
    np_rng = np.random.default_rng([seed, rank, it]); py_rng = random.Random seeded with np_rng's first draw of [0, 2^62).
    Nothing is taken from the global generators, and no generator state has to be saved for a resume."""
    np_rng = np.random.default_rng([int(seed), int(rank), int(it)])
    return np_rng, random.Random(int(np_rng.integers(0, 1 << 62)))


def step_boxes(n: int, h: int, w: int, ratio: float, seed: int, rank: int, it: int, per: str = "batch") -> List[Box]:
    """the n boxes of one training step: `per` "batch" = one box for all samples (CutMix.__call__), "sample" = one draw per sample in
    sample order (augmentation())"""
    if per not in ("batch", "sample"):
        raise ValueError(f"cutmix_boxes must be 'batch' or 'sample', got {per!r}")
    np_rng, py_rng = step_generators(seed, rank, it)
    if per == "batch":
        return [draw_box(h, w, ratio, np_rng, py_rng)] * n
    return [draw_box(h, w, ratio, np_rng, py_rng) for _ in range(n)]


def mix_boxes(t: torch.Tensor, boxes: Sequence[Box], mode: str = "mix", fill=0) -> torch.Tensor:
    """out[s] = t[s] outside boxes[s]; inside, t[(s + 1) % n] ("mix") or `fill` ("fill").  t: (n, P, H, W) or (n, H, W); a new tensor.
    On the GPU: one launch of the box-mix kernel; on the CPU: a selection with torch ops."""
    if t.is_cuda:
        return _hip.box_mix(_dense(t), boxes, mode=mode, fill=fill)
    if len(boxes) != t.shape[0]:
        raise ValueError(f"one box per sample required: {t.shape[0]} samples, {len(boxes)} boxes")
    inside = torch.stack([box_mask(t.shape[-2:], b) == 0 for b in boxes])
    if t.dim() == 4:
        inside = inside[:, None]
    other = torch.roll(t, -1, 0) if mode == "mix" else torch.full_like(t, fill)
    return torch.where(inside, other, t)


class _BoxAug:
    """what CutMix and CutOut share: the ratio, the mask draw and the memory of which box each mask it handed out holds"""

    def __init__(self, ratio: float):
        self.ratio = ratio
        self._made: list = []                   # (weakref(mask), mask._version, box) of the masks this object made

    def _make_mask(self, img_size: Iterable[int]) -> torch.Tensor:
        img_size = tuple(img_size)
        box = draw_box(img_size[0], img_size[1], self.ratio)
        return self._remember(box_mask(img_size, box), box)

    def _remember(self, mask: torch.Tensor, box: Box) -> torch.Tensor:
        self._made = [e for e in self._made if e[0]() is not None][-63:]
        self._made.append((weakref.ref(mask), mask._version, box))
        return mask

    def _box_of(self, mask: torch.Tensor) -> Optional[Box]:
        for ref, version, box in self._made:
            if ref() is mask and mask._version == version:
                return box
        return None

    def _own_mask(self, batch: torch.Tensor) -> torch.Tensor:
        mask = self._make_mask(batch.shape[-2:])
        box = self._box_of(mask)
        moved = mask.to(batch.device)
        return moved if moved is mask else self._remember(moved, box)


class CutMix(_BoxAug):
    """data/augmentations.py:44-73: mixed[i] = batch[i] * mask + batch[(i + 1) % B] * (1 - mask) with ONE box for the batch.
    `__call__(batch, mask=None) -> (mixed, mask)`; hand the returned mask back in to mix the pseudo targets with the same box
    (deprecated/train_vqpt_easyhard_aug.py:119-123).  GPU batches take the kernel whenever the mask is one this object made (it
    remembers the box); a mask from elsewhere is applied with tensor ops on the batch's device -- correct, just not the kernel."""

    def __call__(self, batch: torch.Tensor, mask: Optional[torch.Tensor] = None):
        if mask is None:
            mask = self._own_mask(batch)
        box = self._box_of(mask)
        if batch.is_cuda and box is not None and batch.dim() in (3, 4) and batch.dtype in _hip.BOX_MIX_DTYPES and tuple(batch.shape[-2:]) == tuple(mask.shape):
            return _hip.box_mix(_dense(batch), [box] * batch.shape[0], mode="mix"), mask
        mask = mask.to(batch.device)
        return batch * mask + torch.roll(batch, -1, 0) * (1 - mask), mask


class CutOut(_BoxAug):
    """data/augmentations.py:75-104.  The reference's CutOut.__call__ cannot run: it reads the builtin `input` instead of its argument
    and calls _make_mask with a stray second argument.  This is its evident intent: aug[i] = batch[i] * mask, one box for the batch."""

    def __call__(self, batch: torch.Tensor, mask: Optional[torch.Tensor] = None):
        if mask is None:
            mask = self._own_mask(batch)
        box = self._box_of(mask)
        if batch.is_cuda and box is not None and batch.dim() in (3, 4) and batch.dtype in _hip.BOX_MIX_DTYPES and tuple(batch.shape[-2:]) == tuple(mask.shape):
            return _hip.box_mix(_dense(batch), [box] * batch.shape[0], mode="fill", fill=0), mask
        mask = mask.to(batch.device)
        return batch * mask, mask


aug_dict = {"cutmix": CutMix, "cutout": CutOut}             # data/__init__.py:2-4, plus "cutout"


def make_aug(aug_cfg):
    """data/__init__.py:5-7: aug_dict[name](**the other keys).  (The reference pops "name" out of the caller's dictionary; this
    works on a copy.)"""
    kw = dict(aug_cfg)
    return aug_dict[kw.pop("name")](**kw)


def augmentation(input: torch.Tensor, label: torch.Tensor, logits: torch.Tensor, aug_cfg):
    """data/augmentations.py:11-30: the batch function, ONE BOX PER SAMPLE (drawn in sample order from the global generators, as the
    reference's per-sample make_cutout_mask calls do); aug_cfg has `name` ("cutmix" | "cutout") and `ratio`.
      cutmix: each of input / label / logits mixed with the partner (i + 1) % B inside the sample's box;
      cutout: input and logits zeroed, label set to the ignore index 255 inside the box.
    GPU tensors: one kernel call per tensor.  Two deviations from the reference: its cutout branch writes 255 into the CALLER's
    `label` in place (and then fails on an `unsqueeze()` without argument) -- here `label` is never written, the cut-out labels are a
    copy; and an unknown name raises instead of returning three empty concatenations."""
    get = aug_cfg.get if isinstance(aug_cfg, dict) else lambda k: getattr(aug_cfg, k)
    name, ratio = get("name"), get("ratio")
    if name not in ("cutmix", "cutout"):
        raise ValueError(f"augmentation: unknown name {name!r}")
    h, w = input.shape[-2:]
    boxes = [draw_box(h, w, ratio) for _ in range(input.shape[0])]
    if input.is_cuda:
        if name == "cutmix":
            return tuple(_hip.box_mix(_dense(t), boxes, mode="mix") for t in (input, label, logits))
        return (_hip.box_mix(_dense(input), boxes, mode="fill", fill=0), _hip.box_mix(_dense(label), boxes, mode="fill", fill=255),
                _hip.box_mix(_dense(logits), boxes, mode="fill", fill=0))
    masks = [box_mask((h, w), b) for b in boxes]            # CPU: the reference's arithmetic, sample by sample
    n = input.shape[0]
    if name == "cutmix":
        return tuple(torch.cat([(t[i] * masks[i] + t[(i + 1) % n] * (1 - masks[i])).unsqueeze(0) for i in range(n)], dim=0)
                     for t in (input, label, logits))
    lab = label.clone()
    for i in range(n):
        lab[i][(1 - masks[i]).bool()] = 255
    return (torch.cat([(input[i] * masks[i]).unsqueeze(0) for i in range(n)], dim=0), lab,
            torch.cat([(logits[i] * masks[i]).unsqueeze(0) for i in range(n)], dim=0))
