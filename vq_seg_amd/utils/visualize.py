"""Colour maps and example sheets (reference: utils/visualize.py), and the native entry `render_sheet`.

The reference composes its sheets on the host in float64 numpy from logits and images copied off the device, and hands the float
result to `plt.imsave`.  Here the same names take either

  * numpy arrays / CPU tensors -- composed in float64 numpy with the reference's arithmetic (`colormap[label]`, concatenation,
    `input * (1 - alpha) + pred * alpha`, clip), or
  * device tensors -- `nnf.resize_argmax` (labels at the display size, 1 byte per pixel) + `nnf.render_sheet` (vqseg_render_sheet_u8:
    labels, targets and the image become the sheet's RGB bytes in one pass); only the uint8 sheet crosses to the host.

Deviations from the reference, all on purpose:
  1. Every function returns **uint8** -- `(H, W, 3)` for sheets, `(N, H, W, 3)` for the colour maps -- equal to what `plt.imsave`
     writes from the reference's float result (matplotlib's `to_rgba(bytes=True)` is `(x * 255).astype(uint8)`, i.e. floor), not
     the float array.  `save_img` and wandb take a uint8 array as they take the float one.
  2. `pred_to_detailed_colormap` takes the class count from the logits' channel dimension, not from `len(np.unique(target))`
     (the reference raises unless the target happens to hold exactly 3 distinct values), and colours a pixel "wrong" wherever
     `pred != target`.  The "wrong" colours come from rows C .. 2 C - 1 of `colormap` when it has them, else from DEFAULT_PALETTE's.
  3. `resize_factor` is `None` or `0.5`; anything else is NotImplementedError.  0.5 is a 2 x 2 box mean of the float sheet, which
     is what `cv2.resize(fx=fy=0.5, INTER_LINEAR)` computes at even sizes (the half-pixel-centre rule puts every sample exactly
     between two pixels in each direction); cv2 is not a dependency of this package and that reading is not measured against it.
     Odd sheet heights or widths raise ValueError.  On device tensors 0.5 also needs an even image width (the labelled and the
     unlabelled half of `make_example_img` are two launches into one canvas).
  4. A target outside [0, C) (the ignore value 255) takes the palette's ignore colour (white by default); the reference raises.
The saliency / SLIC / self-supervision variants are not here: their networks are out of scope.

This module imports neither matplotlib, PIL nor cv2 and does not touch the GPU at import time.
"""
import os
from typing import List

import numpy as np
import torch

_CLASS = [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
_WRONG = [[0.5, 0.5, 0.5], [230 / 255, 145 / 255, 56 / 255], [1.0, 217 / 255, 102 / 255], [0.6, 0.9, 0.6]]    # test_detailviz.py:129 (+ a 4th)
_IGNORE = [1.0, 1.0, 1.0]
_COLORMAP = np.array(_CLASS[:3])                       # the reference's default `colormap`
GAP = 20                                               # the white gap of make_example_img, in pixels


def default_palette(num_classes: int = 3) -> np.ndarray:
    """(2 C + 1, 3) float64: C class colours (black, blue, red[, green]), C "wrong" colours (gray, orange, yellow[, pale green]), the
    ignore colour (white)"""
    if not 2 <= int(num_classes) <= 4:
        raise ValueError(f"num_classes must be 2..4, got {num_classes}")
    c = int(num_classes)
    return np.array(_CLASS[:c] + _WRONG[:c] + [_IGNORE], dtype=np.float64)


DEFAULT_PALETTE = default_palette(3)


# ---------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------
def _on_device(*xs) -> bool:
    return any(torch.is_tensor(x) and x.is_cuda for x in xs)


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _t(x):
    return x if torch.is_tensor(x) or x is None else torch.as_tensor(np.asarray(x))


def _u8(x) -> np.ndarray:
    """what plt.imsave writes from a float image: floor(clip(x, 0, 1) * 255); a NaN gives 0.  uint8 passes through."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x
    return (np.clip(np.nan_to_num(x.astype(np.float64), nan=0.0), 0.0, 1.0) * 255).astype(np.uint8)


def _palette(colormap, c: int) -> np.ndarray:
    """the (2 C + 1, 3) palette a reference-style `colormap` of C, 2 C or 2 C + 1 rows stands for"""
    cm = np.asarray(_np(colormap), dtype=np.float64)
    if cm.ndim != 2 or cm.shape[1] != 3 or len(cm) < c:
        raise ValueError(f"colormap must have at least {c} rows of 3, got shape {cm.shape}")
    base = default_palette(c)
    wrong = cm[c:2 * c] if len(cm) >= 2 * c else base[c:2 * c]
    ignore = cm[2 * c:2 * c + 1] if len(cm) > 2 * c else base[2 * c:]
    return np.concatenate([cm[:c], wrong, ignore], axis=0)


def _classes(colormap, logits=None) -> int:
    if logits is not None:
        return int(logits.shape[1])
    n = len(colormap)
    return n if n <= 4 else n // 2


def _half(sheet: np.ndarray) -> np.ndarray:
    if sheet.shape[0] % 2 or sheet.shape[1] % 2:
        raise ValueError(f"resize_factor=0.5 needs a sheet of even height and width, got {sheet.shape[0]} x {sheet.shape[1]}")
    return (sheet[0::2, 0::2] + sheet[0::2, 1::2] + sheet[1::2, 0::2] + sheet[1::2, 1::2]) / 4.0


def _factor(resize_factor) -> bool:
    if resize_factor is None:
        return False
    if resize_factor == 0.5:
        return True
    raise NotImplementedError(f"resize_factor is None or 0.5 (a 2 x 2 box mean), got {resize_factor!r}")


def _nearest(target: np.ndarray, size) -> np.ndarray:
    """ATen's nearest rule: src = min(int(dst * float32(in / out)), in - 1); the identity when the sizes agree"""
    ht, wt = target.shape[-2:]
    ho, wo = size
    if (ht, wt) == (ho, wo):
        return target
    ys = np.minimum((np.arange(ho, dtype=np.float32) * (np.float32(ht) / np.float32(ho))).astype(np.int64), ht - 1)
    xs = np.minimum((np.arange(wo, dtype=np.float32) * (np.float32(wt) / np.float32(wo))).astype(np.int64), wt - 1)
    return target[:, ys][:, :, xs]


def _sheet_float(panels, size, c, palette, image=None, label=None, target=None, fill=(1.0, 1.0, 1.0), alpha=0.4) -> np.ndarray:
    """the float64 sheet (B * Ho, width, 3) of numpy sources, with the reference's arithmetic"""
    from .. import nnf
    ho, wo = size
    layout, _ = nnf.sheet_layout(panels, wo)
    palette = np.asarray(palette, dtype=np.float64)
    if palette.shape != (2 * c + 1, 3):
        raise ValueError(f"the palette of {c} classes has {2 * c + 1} rows of 3 (class, wrong, ignore), got shape {palette.shape}")
    img = lab = tgt = None
    if image is not None:
        image = np.asarray(image)
        if tuple(image.shape[-2:]) != (ho, wo):                                   # as test_detailviz.py:125 does on the host
            image = torch.nn.functional.interpolate(torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)), size=(ho, wo),
                                                    mode="bilinear", align_corners=False).numpy()
        img = batch_to_grid(image.astype(np.float64))
    if label is not None:
        lab = np.asarray(label).astype(np.int64)
        lab = np.where((lab >= 0) & (lab < c), lab, 2 * c)
    if target is not None:
        tgt = _nearest(np.asarray(target).astype(np.int64), (ho, wo))
    need = {"image": (img,), "target": (tgt,), "pred": (lab,), "detail": (lab, tgt), "mix_pred": (img, lab), "mix_detail": (img, lab, tgt), "fill": ()}
    rows = next(x.shape[0] * (1 if x is img else ho) for x in (img, lab, tgt) if x is not None)
    parts = []
    for kind, _x0, width in layout:
        if any(s is None for s in need[kind]):
            raise ValueError(f"panel {kind!r} needs a source that was not given")
        if kind == "fill":
            parts.append(np.ones((rows, width, 3), dtype=np.float64) * np.asarray(fill, dtype=np.float64))
            continue
        if kind == "image":
            parts.append(img)
            continue
        if kind == "target":
            idx = np.where((tgt >= 0) & (tgt < c), tgt, 2 * c)
        elif kind in ("pred", "mix_pred"):
            idx = lab
        else:
            idx = np.where(lab == 2 * c, lab, np.where(lab != tgt, lab + c, lab))
        colour = batch_to_grid(palette[idx], transpose=False)
        parts.append(np.clip(img * (1 - alpha) + colour * alpha, 0, 1) if kind.startswith("mix") else colour)
    return np.concatenate(parts, axis=1)


def _label_of(pred, size=None):
    """(N, C, H, W) logits -> arg-max labels (a device tensor goes through the fused kernel), an integer (N, H, W) map as it is"""
    if torch.is_tensor(pred) and pred.is_cuda:
        if pred.dim() == 3:
            return pred.to(torch.uint8)
        from .. import nnf
        return nnf.resize_argmax(pred.float(), tuple(pred.shape[-2:]) if size is None else size)[0]
    pred = _np(pred)
    if pred.ndim == 4 and size is not None and tuple(pred.shape[-2:]) != tuple(size):      # logits below the display size: resized first
        from .. import nnf
        return nnf.resize_argmax(torch.from_numpy(np.ascontiguousarray(pred, dtype=np.float32)), size)[0].numpy()
    return pred if pred.ndim == 3 else np.argmax(pred, axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# the native entry
# ---------------------------------------------------------------------------------------------------------------------------
def render_sheet(panels, image=None, logits_or_label=None, target=None, size=None, palette=None, alpha=0.4, half=False, fill=(1.0, 1.0, 1.0),
                 flips=None, num_classes=None, out=None) -> torch.Tensor:
    """A panel sheet as a uint8 (rows, cols, 3) tensor on the sources' device.  `panels`, left to right: "image", "target", "pred",
    "detail", "mix_pred", "mix_detail", ("fill", width) (nnf.render_sheet).  `image` (B, 3, h, w) float in [0, 1]; `logits_or_label`:
    (B, C, h', w') logits, a list of such views with `flips` (nnf.resize_argmax) or a (B, Ho, Wo) integer label map; `target`
    (B, Ht, Wt) integer labels at any size; `size` (Ho, Wo): the display size of every panel (default: the image's, else the
    label's); `palette` (2 C + 1, 3) (default: default_palette(C)); `half`: the sheet halved by 2 x 2 box means.  Image i takes the
    rows i Ho .. (i + 1) Ho - 1 of every panel.  Device tensors: one resize_argmax launch (for logits) and one render launch into
    `out` (optional: a (rows, cols, 3) uint8 view); numpy arrays / CPU tensors: float64 numpy."""
    image, target = _t(image), _t(target)
    views = logits_or_label
    if views is not None:
        views = [_t(v) for v in views] if isinstance(views, (list, tuple)) else _t(views)
    first = views[0] if isinstance(views, list) else views
    if size is None:
        ref = image if image is not None else first if first is not None else target
        if ref is None:
            raise ValueError("render_sheet: nothing to draw: give an image, logits / labels or a target")
        size = tuple(ref.shape[-2:])
    size = (int(size[0]), int(size[1]))
    is_logits = first is not None and first.dim() == 4
    c = int(first.shape[1]) if is_logits else int(num_classes) if num_classes is not None else (len(palette) - 1) // 2 if palette is not None else 3
    palette = default_palette(c) if palette is None else np.asarray(_np(palette), dtype=np.float64)
    from .. import nnf
    label = None
    if first is not None:
        if is_logits and not isinstance(views, list) and not first.is_cuda and tuple(first.shape[-2:]) == size and not flips:
            label = torch.from_numpy(np.argmax(_np(first), axis=1).astype(np.uint8))       # the reference's own line, in the logits' own type
        elif is_logits:
            label = nnf.resize_argmax([v.float() for v in views] if isinstance(views, list) else views.float(), size, flips=flips)[0]
        else:
            if tuple(first.shape[-2:]) != size:
                raise ValueError(f"render_sheet: a label map must have the display size {size}, got {tuple(first.shape[-2:])}")
            label = first.to(torch.uint8)
    if _on_device(image, label, target, out):
        return nnf.render_sheet(panels, size, c, palette, image=None if image is None else image.float(), pred=label, target=target, fill=fill,
                                alpha=alpha, half=half, out=out)
    sheet = _sheet_float(panels, size, c, palette, None if image is None else _np(image), None if label is None else _np(label),
                         None if target is None else _np(target), fill, alpha)
    sheet = torch.from_numpy(_u8(_half(sheet) if half else sheet))
    if out is not None:
        out.copy_(sheet)
        return out
    return sheet


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's names
# ---------------------------------------------------------------------------------------------------------------------------
def _maps(kind, pred, target, colormap, c) -> np.ndarray:
    """(N, H, W, 3) uint8 colour map of one panel kind"""
    src = pred if pred is not None else target
    n, (h, w) = src.shape[0], tuple(src.shape[-2:])
    sheet = render_sheet([kind], logits_or_label=pred, target=target, size=(h, w), palette=_palette(colormap, c), num_classes=c)
    return _np(sheet).reshape(n, h, w, 3)


def pred_to_colormap(pred, colormap):
    """(N, C, H, W) logits -> (N, H, W, 3) uint8: `colormap[argmax]`"""
    return _maps("pred", _t(pred), None, colormap, _classes(colormap, pred))


def pred_to_detailed_colormap(pred, target, colormap):
    """as pred_to_colormap, a pixel whose arg-max differs from `target` in the "wrong" colour of its class (deviation 2 above)"""
    return _maps("detail", _t(pred), _t(target), colormap, _classes(colormap, pred))


def target_to_colormap(target, colormap):
    """(N, H, W) labels -> (N, H, W, 3) uint8: `colormap[target]`"""
    return _maps("target", None, _t(target), colormap, _classes(colormap))


def batch_to_grid(array: np.ndarray, transpose=True):
    """(N, C, H, W) -- or (N, H, W, C) with transpose=False -- -> (N * H, W, C): the batch stacked vertically"""
    array = _np(array)
    array = array.transpose(0, 2, 3, 1) if transpose else array
    return np.squeeze(np.concatenate(np.split(array, len(array), axis=0), axis=1), axis=0)


def mix_input_pred(input, pred, alpha=0.4):
    """clip(input * (1 - alpha) + pred * alpha, 0, 1) of two float colour arrays as uint8 (a uint8 `pred` counts as pred / 255)"""
    input, pred = _np(input), _np(pred)
    input = input / 255.0 if input.dtype == np.uint8 else input.astype(np.float64)
    pred = pred / 255.0 if pred.dtype == np.uint8 else pred.astype(np.float64)
    return _u8(np.clip(input * (1 - alpha) + pred * alpha, 0, 1))


def make_example_img(l_input, target, pred, ul_input, ul_pred, colormap=_COLORMAP, resize_factor=0.5):
    """[input | target | prediction | 20 px white | 0.6 unlabelled input + 0.4 its prediction], the batch stacked vertically, uint8;
    without the unlabelled pair only the first three panels at full size, as the reference.  Device tensors stay on the device until
    the uint8 sheet is complete: pass the trainer's tensors without detach_numpy."""
    half = _factor(resize_factor)
    c = _classes(colormap, pred)
    palette = _palette(colormap, c)
    labelled = ["image", "target", "pred"]
    size = tuple(l_input.shape[-2:])
    if ul_input is None and ul_pred is None:
        return _np(render_sheet(labelled, l_input, pred, target, size=size, palette=palette))
    if tuple(ul_input.shape[-2:]) != size or ul_input.shape[0] != l_input.shape[0]:
        raise ValueError(f"the labelled and the unlabelled batch must have one shape, got {tuple(l_input.shape)} and {tuple(ul_input.shape)}")
    n, (h, w) = l_input.shape[0], size
    if not _on_device(l_input, target, pred, ul_input, ul_pred):
        sheet = np.concatenate((_sheet_float(labelled + [("fill", GAP)], size, c, palette, _np(l_input), _label_of(pred, size), _np(target)),
                                _sheet_float(["mix_pred"], size, c, palette, _np(ul_input), _label_of(ul_pred, size))), axis=1)
        return _u8(_half(sheet) if half else sheet)
    rows, cols, split = n * h, 4 * w + GAP, 3 * w + GAP
    if half and (rows % 2 or split % 2):
        raise ValueError(f"resize_factor=0.5 on device tensors needs an even sheet height and image width, got {rows} rows, width {w}")
    k = 2 if half else 1
    dev = next(x.device for x in (l_input, target, pred, ul_input, ul_pred) if torch.is_tensor(x) and x.is_cuda)
    to = lambda x: _t(x).to(dev)                         # noqa: E731
    canvas = torch.empty((rows // k, cols // k, 3), dtype=torch.uint8, device=dev)
    render_sheet(labelled + [("fill", GAP)], to(l_input), to(pred), to(target), size=size, palette=palette, half=half, out=canvas[:, :split // k])
    render_sheet(["mix_pred"], to(ul_input), to(ul_pred), size=size, palette=palette, half=half, out=canvas[:, split // k:])
    return canvas.cpu().numpy()


def _test_img(kinds, input, pred, target, colormap):
    c = _classes(colormap, pred)
    input, pred, target = _t(input), _t(pred), _t(target)
    if _on_device(input, pred, target):
        dev = next(x.device for x in (input, pred, target) if x.is_cuda)
        input, pred, target = input.to(dev), pred.to(dev), target.to(dev)
    w = input.shape[-1]
    sheet = _np(render_sheet(["image", "target"] + kinds, input, pred, target, size=tuple(input.shape[-2:]), palette=_palette(colormap, c)))
    return np.ascontiguousarray(sheet[:, :3 * w]), np.ascontiguousarray(sheet[:, 3 * w:])


def make_test_img(input, pred, target, colormap: np.ndarray = _COLORMAP):
    """-> (viz_v1 = [input | target | prediction], viz_v2 = 0.6 input + 0.4 prediction), uint8"""
    return _test_img(["pred", "mix_pred"], input, pred, target, colormap)


def make_test_detailed_img(input, pred, target, colormap: np.ndarray = _COLORMAP):
    """make_test_img with the detailed prediction: a wrong pixel in its class's second colour (test_detailviz.py:129)"""
    return _test_img(["detail", "mix_detail"], input, pred, target, colormap)


def save_img(img_dir: str, filename: str, img: np.ndarray):
    """write `img` (uint8, or float in [0, 1] quantised as plt.imsave does) as an image file; the format follows the extension"""
    from PIL import Image                                # the decoder library of data.dataset.BaseDataset; not at import time
    Image.fromarray(np.ascontiguousarray(_u8(_np(img)))).save(os.path.join(img_dir, filename))


def save_img_list(img_dir, filename_list: List[str], img_list: List[np.ndarray]):
    for img, filename in zip(img_list, filename_list):
        save_img(img_dir, filename, img)
