"""CutMix / CutOut (reference: data/augmentations.py:11-104; registered in data/__init__.py:1-7; driven by
deprecated/train_vqpt_easyhard_aug.py:90,119-123).  The strong-augmentation half of cross pseudo supervision: the unlabelled
training forwards see box-mixed images, and the pseudo targets are mixed with the same box.

The box draw is the reference's, draw for draw (`draw_box`), so a seeded run of the reference's augmentation code and of this one
pick the same boxes.  CPU tensors take the reference's arithmetic (batch * mask + partner * (1 - mask)) with torch ops; tensors on
the GPU take ONE HIP pass per tensor (`_hip.box_mix`, vqseg_box_mix_f) that selects by bits.  The two agree on every finite value
(0 / 1 masks make the arithmetic a selection); they differ only where arithmetic is not a selection: the reference turns -0.0 into
+0.0 and spreads a NaN / inf of the partner over the whole image (x * 1 + nan * 0), the kernel passes every bit pattern through.

Similarity transforms (reference: data/augmentations.py:108-148; driven by deprecated/train_vqpt_easyhard_aug.py:90-123 as the EASY
augmentation: the pseudo-label forwards see a flipped / rotated batch, and inverse_similarity_transform brings their outputs back into
the clean frame).  What is the reference's: the two names and signatures, the ten codes, and the draws in their order -- one
random.randint(0, 9), then, for every code but 1 and 2, one uniform angle of [0, 90) from torch's global generator
(RandomRotation.get_params, restated from torchvision's source: torchvision is not a dependency).  What is evident intent: the
reference's forward rotations call TF.rotate and DROP the result (codes 3-8 return their input, or nothing but the flip), codes 4 / 6 / 8
negate the angle and then pass its negation again, and codes 0 and 9 return a drawn angle that the inverse would then rotate by.  Built
here: code 1 / 2 = horizontal / vertical flip; 3 / 4 = rotation by +a / -a; 5 / 6 = horizontal flip, then rotation by +a / -a; 7 / 8 =
vertical flip, then rotation; 0 and 9 = identity.  The angle returned is signed (negative for 4 / 6 / 8) and 0.0 for codes 0, 1, 2 and 9,
so inverse_similarity_transform(similarity_transform(x)) is the exact matrix inverse for every code.  A rotation is TF.rotate's on
tensors -- grid_sample, align_corners=False, zero fill, positive = counter-clockwise as displayed -- restated in pixel space
(`similarity_matrices`, `warp_batch`; vqseg_affine_warp_f on the GPU).  Where the two differ on purpose: the reference's inverse
interpolates integer class maps bilinearly, which invents classes between two labels; integer and bool tensors here take the NEAREST
source pixel (and `fill` outside the image).  Flips, quarter turns on square images and the identity pass every bit pattern through,
on either device.

Photometric strong augmentation (no reference counterpart: its hard augmentation stops at CutMix; this is the colour half of the
FixMatch / UniMatch strong view that deprecated/train_vqpt_easyhard_aug.py and deprecated/train_UNIMatch.py belong to).  What is
defined HERE, once, in include/vqseg.h (vqseg_photometric_f) and restated in float64 by tests/photometric_cases.py: six ops per sample
in a fixed order -- brightness, contrast (about the sample's mean gray), saturation, hue (hexcone RGB <-> HSV), grayscale, Gaussian
blur (radius ceil(3 sigma) <= 8, reflect-101 borders, float32 taps made in float64 on the host) -- all in float32, an op at its
identity value skipped, an all-identity row a copy of the bits.  Why fixed: a step's view must be a pure function of (seed, rank,
iteration), and one order of ops is one kernel; the draws (`draw_photometric`, `step_photometric`) take exactly eight uniforms per
sample under a generator key of their own, so neither the CutMix boxes nor the similarity transforms of a step move.  What is NOT
torchvision's or PIL's, and is not claimed to be: torchvision's ColorJitter applies its four ops in a random order and blends
contrast about the mean of ITS grayscale after ITS rounding, PIL's GaussianBlur is a box approximation; neither is a dependency, and
the yardstick is the float64 restatement.  GPU tensors take the photometric kernel (`_hip.photometric`), CPU tensors the same
definition with float32 torch ops (`photometric`); the two agree within float32 rounding, and exactly on identity rows.
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


# ---- similarity transforms (flip / rotation): the easy augmentation ---------------------------------------------------------------

_FLIP = {1: (-1.0, 1.0), 2: (1.0, -1.0), 5: (-1.0, 1.0), 6: (-1.0, 1.0), 7: (1.0, -1.0), 8: (1.0, -1.0)}     # code -> diag(sx, sy) of its flip
_QUARTER = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}                          # angle mod 360 -> exact (cos, sin)


def similarity_matrices(codes, angles, inverse: bool = False) -> np.ndarray:
    """float32 (n, 6) rows (M00, M01, 0, M10, M11, 0) for `warp_batch` / _hip.affine_warp: the matrix that maps an OUTPUT pixel's
    offset from the image centre to its SOURCE pixel's.  `codes`: the reference's transform codes 0-9; `angles`: SIGNED degrees, as
    similarity_transform returns them (negative for codes 4 / 6 / 8; ignored for 0, 1, 2 and 9).  A rotation by a (positive =
    counter-clockwise as displayed, TF.rotate) samples xs = cos a dx - sin a dy, ys = sin a dx + cos a dy; "flip, then rotate" is
    F R(a), its inverse -- rotate by -a, then the same flip -- R(-a) F.  Computed in float64; multiples of 90 degrees get exact
    0 / +-1 entries, so flips and quarter turns are exact permutations of the pixels."""
    codes = np.atleast_1d(np.asarray(codes)).astype(np.int64)
    angles = np.atleast_1d(np.asarray(angles, dtype=np.float64))
    if codes.ndim != 1 or codes.shape != angles.shape:
        raise ValueError(f"similarity_matrices: one code and one angle per sample required, got shapes {codes.shape} and {angles.shape}")
    if codes.size and (codes.min() < 0 or codes.max() > 9):
        raise ValueError("similarity_matrices: codes must lie in 0..9")
    if not np.isfinite(angles).all():
        raise ValueError("similarity_matrices: an angle is not finite")
    out = np.zeros((codes.size, 6), dtype=np.float64)
    for i, (c, a) in enumerate(zip(codes.tolist(), angles.tolist())):
        a = 0.0 if c in (0, 1, 2, 9) else (-a if inverse else a)
        cs = _QUARTER.get(a % 360.0)
        co, si = cs if cs is not None else (float(np.cos(np.deg2rad(a))), float(np.sin(np.deg2rad(a))))
        rot = np.array([[co, -si], [si, co]])
        flip = np.diag(_FLIP.get(c, (1.0, 1.0)))
        m = rot @ flip if inverse else flip @ rot
        out[i, 0:2], out[i, 3:5] = m[0], m[1]
    return (out + 0.0).astype(np.float32)                   # (+ 0.0: no negative zeros among the entries)


def _warp_torch(t: torch.Tensor, mats: np.ndarray, mode: str, fill) -> torch.Tensor:
    """the kernel's arithmetic with torch ops (CPU tensors, and whatever the kernel does not take): the same float32 source
    coordinates in the same order, the same tap order, zero-weight and outside taps left out, whole source pixels taken by value"""
    n, (h, w) = t.shape[0], t.shape[-2:]
    dev = t.device
    m = torch.as_tensor(mats, dtype=torch.float32, device=dev)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    dx = (torch.arange(w, dtype=torch.float32, device=dev) - cx)[None, None, :]
    dy = (torch.arange(h, dtype=torch.float32, device=dev) - cy)[None, :, None]
    col = [m[:, k, None, None] for k in range(6)]
    xs = (col[0] * dx + col[1] * dy) + cx                  # separate ops: no fused multiply-add
    ys = (col[3] * dx + col[4] * dy) + cy
    xs = torch.nan_to_num(xs, nan=-2.0).clamp(-2.0, w + 1.0)           # far outside is outside (and stays convertible to an index)
    ys = torch.nan_to_num(ys, nan=-2.0).clamp(-2.0, h + 1.0)
    flat = t.reshape(n, -1, h * w)                          # (n, P, h w); P = 1 for 3-D maps
    planes = flat.shape[1]
    # whole pixels are moved as BITS (an integer view of the same width): torch's selections may pass a bfloat16 through float32 and
    # lose a NaN's payload on the way
    as_bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    bits = flat.view(as_bits) if (t.is_floating_point() or t.dtype == torch.bool) else flat

    def tap(of, xi, yi):
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        at = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).reshape(n, 1, h * w).expand(n, planes, h * w)
        return torch.gather(of, 2, at), inside.reshape(n, 1, h * w)

    if mode == "nearest":
        v, inside = tap(bits, torch.round(xs).long(), torch.round(ys).long())    # round half to even
        fill_bits = torch.tensor([fill], dtype=t.dtype).view(bits.dtype).to(dev)
        return torch.where(inside, v, fill_bits).view(t.dtype).reshape(t.shape)
    xf, yf = torch.floor(xs), torch.floor(ys)
    fx, fy = xs - xf, ys - yf
    x0, y0 = xf.long(), yf.long()
    acc = torch.zeros(flat.shape, dtype=torch.float32, device=dev)
    for wgt, xi, yi in (((1.0 - fy) * (1.0 - fx), x0, y0), ((1.0 - fy) * fx, x0 + 1, y0), (fy * (1.0 - fx), x0, y0 + 1), (fy * fx, x0 + 1, y0 + 1)):
        v, inside = tap(flat, xi, yi)
        wgt = wgt.reshape(n, 1, h * w)
        acc = acc + torch.where(inside & (wgt != 0), wgt * v.float(), torch.zeros((), dtype=torch.float32, device=dev))
    v00, in00 = tap(bits, x0, y0)
    whole = ((fx == 0) & (fy == 0)).reshape(n, 1, h * w)
    return torch.where(whole, torch.where(in00, v00, torch.zeros_like(v00)), acc.to(t.dtype).view(as_bits)).view(t.dtype).reshape(t.shape)


def warp_batch(t: torch.Tensor, matrices, mode: str = "bilinear", fill=0) -> torch.Tensor:
    """out[s] = t[s] resampled through matrices[s] (rows of `similarity_matrices`); t: (n, P, H, W) or (n, H, W); a new tensor.
    `mode` "bilinear" (floating tensors; zero padding) or "nearest" (any dtype; `fill` outside the image).  On the GPU: one launch of the
    affine-warp kernel for the dtypes it takes; CPU tensors and the rest: the same arithmetic with torch ops."""
    if mode not in ("bilinear", "nearest"):
        raise ValueError(f"warp_batch: mode must be 'bilinear' or 'nearest', got {mode!r}")
    if t.dim() not in (3, 4):
        raise ValueError("warp_batch: a (n, P, H, W) or (n, H, W) tensor required")
    mats = np.ascontiguousarray(matrices, dtype=np.float32)
    if mats.shape != (t.shape[0], 6):
        raise ValueError(f"one matrix row per sample required: {t.shape[0]} samples, matrices of shape {mats.shape}")
    if mode == "bilinear" and not t.is_floating_point():
        raise ValueError(f"warp_batch: bilinear needs a floating tensor, got {t.dtype} (integer maps take mode='nearest')")
    if t.is_cuda and t.dtype in (_hip.AFFINE_WARP_BILINEAR_DTYPES if mode == "bilinear" else _hip.AFFINE_WARP_NEAREST_DTYPES):
        return _hip.affine_warp(_dense(t), mats, mode=mode, fill=fill)
    if not np.isfinite(mats).all() or mats[:, (2, 5)].any():
        raise ValueError("warp_batch: matrix entries must be finite and the translation slots 0")
    return _warp_torch(t, mats, mode, fill)


def _similarity(input: torch.Tensor, aug: int, angle: float, inverse: bool, fill=0) -> torch.Tensor:
    """one transform for the whole of `input` (..., H, W): a (n, P, H, W) or (n, H, W) batch as it is, a single (H, W) map as a batch of one"""
    if input.dim() < 2:
        raise ValueError("similarity transforms need a (..., H, W) tensor")
    batched = input if input.dim() in (3, 4) else input[None] if input.dim() == 2 else input.flatten(0, -4)
    n = batched.shape[0]
    mats = similarity_matrices([int(aug)] * n, [float(angle)] * n, inverse=inverse)
    mode = "bilinear" if input.is_floating_point() else "nearest"
    return warp_batch(batched, mats, mode=mode, fill=fill).reshape(input.shape)


def similarity_transform(input: torch.Tensor, aug: Optional[int] = None):
    """data/augmentations.py:108-134 as it is meant (module docstring): -> (output, aug, angle).  `aug` None draws
    random.randint(0, 9) from Python's global generator; every code but 1 and 2 then draws one angle of [0, 90) from torch's global
    generator -- also codes 0 and 9, which do not use it (the reference's order of draws).  The angle returned is signed (negative
    for 4 / 6 / 8), and 0.0 for codes 0, 1, 2, 9.  `input`: (..., H, W); floating tensors are resampled bilinearly with zero fill,
    integer and bool tensors take the nearest source pixel."""
    if aug is None:
        aug = random.randint(0, 9)
    aug = int(aug)
    if not 0 <= aug <= 9:
        raise ValueError(f"similarity_transform: aug must lie in 0..9, got {aug}")
    angle = 0.0
    if aug not in (1, 2):
        drawn = float(torch.empty(1).uniform_(0.0, 90.0).item())        # RandomRotation.get_params([0., 90.])
        if aug in (3, 5, 7):
            angle = drawn
        elif aug in (4, 6, 8):
            angle = -drawn
    return _similarity(input, aug, angle, inverse=False), aug, angle


def inverse_similarity_transform(input: torch.Tensor, aug: int, angle: float, fill=0) -> torch.Tensor:
    """data/augmentations.py:136-148: the transform that undoes similarity_transform(., aug) -> (., aug, angle): rotate by -angle,
    then the code's flip.  Floating tensors: bilinear, zero fill.  Integer and bool tensors (pseudo labels): NEAREST, `fill` outside
    the image (255 = the ignore index) -- a deviation on purpose, see the module docstring."""
    aug = int(aug)
    if not 0 <= aug <= 9:
        raise ValueError(f"inverse_similarity_transform: aug must lie in 0..9, got {aug}")
    return _similarity(input, aug, angle, inverse=True, fill=fill)


def step_transforms(n: int, seed: int, rank: int, it: int, per: str = "batch", codes: Sequence[int] = tuple(range(10)),
                    max_angle: float = 90.0) -> Tuple[List[int], List[float]]:
    """the n (code, signed angle) pairs of one training step as a pure function of (seed, rank, iteration): `per` "batch" = one
    transform for all samples (the reference draws once per batch), "sample" = one per sample in sample order.  Per transform: the
    code uniformly from `codes`, then -- for every code but 1 and 2, as similarity_transform draws -- an angle uniformly of
    [0, max_angle), signed as similarity_transform signs it.  The generator is np.random.default_rng([seed, rank, it, 1]): a key
    `step_generators` never uses, so a step's CutMix boxes do not depend on this option, and nothing is taken from the global
    generators."""
    if per not in ("batch", "sample"):
        raise ValueError(f"easy_aug_per must be 'batch' or 'sample', got {per!r}")
    codes = [int(c) for c in codes]
    if not codes or min(codes) < 0 or max(codes) > 9:
        raise ValueError(f"step_transforms: codes must be a non-empty selection of 0..9, got {codes!r}")
    rng = np.random.default_rng([int(seed), int(rank), int(it), 1])

    def draw():
        c = codes[int(rng.integers(0, len(codes)))]
        a = 0.0 if c in (1, 2) else float(rng.uniform(0.0, float(max_angle)))
        return c, (a if c in (3, 5, 7) else -a if c in (4, 6, 8) else 0.0)

    pairs = [draw()] * int(n) if per == "batch" else [draw() for _ in range(int(n))]
    return [c for c, _a in pairs], [a for _c, a in pairs]


# ---- photometric strong augmentation (colour jitter, grayscale, blur): the hard augmentation's colour half --------------------------

PhotometricRow = Tuple[float, float, float, float, float, float]       # (b, c, sat, hue, gray, sigma)
IDENTITY_PHOTOMETRIC: PhotometricRow = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
PHOTOMETRIC_DEFAULTS = dict(jitter=(0.5, 0.5, 0.5, 0.25), jitter_p=0.8, gray_p=0.2, blur_p=0.5, sigma=(0.1, 2.0))     # the FixMatch / UniMatch strong view

photometric_taps = _hip.photometric_taps                    # the 2R + 1 float32 taps of a sigma (float64 on the host, rounded once)


def check_photometric_ranges(jitter, jitter_p, gray_p, blur_p, sigma) -> None:
    """ValueError unless the draw ranges can only give rows the definition admits: jitter = (B, C, S, Hh) with B, C, S in [0, 1] (factors
    1 +- X stay >= 0) and Hh in [0, 0.5]; probabilities in [0, 1]; sigma = (lo, hi) with 0 <= lo <= hi <= 8 / 3 (R = ceil(3 sigma) <= 8)"""
    try:
        jit, sig = tuple(float(v) for v in jitter), tuple(float(v) for v in sigma)
    except (TypeError, ValueError):
        raise ValueError(f"photometric: jitter must be four numbers and sigma two, got {jitter!r} and {sigma!r}") from None
    if len(jit) != 4 or not all(0.0 <= v <= 1.0 for v in jit[:3]) or not 0.0 <= jit[3] <= 0.5:
        raise ValueError(f"photometric: jitter must be (B, C, S, Hh) with B, C, S in [0, 1] and Hh in [0, 0.5], got {jitter!r}")
    for name, p in (("jitter_p", jitter_p), ("gray_p", gray_p), ("blur_p", blur_p)):
        if isinstance(p, bool) or not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"photometric: {name} must be a probability, got {p!r}")
    if len(sig) != 2 or not 0.0 <= sig[0] <= sig[1] <= _hip.PHOTOMETRIC_MAX_RADIUS / 3.0:
        raise ValueError(f"photometric: sigma must be (lo, hi) with 0 <= lo <= hi <= {_hip.PHOTOMETRIC_MAX_RADIUS} / 3, got {sigma!r}")


def draw_photometric(rng, jitter=(0.5, 0.5, 0.5, 0.25), jitter_p: float = 0.8, gray_p: float = 0.2, blur_p: float = 0.5,
                     sigma=(0.1, 2.0)) -> PhotometricRow:
    """one parameter row from EXACTLY eight uniforms u = rng.random(8) of a np.random.Generator, whatever the outcome: jitter on iff
    u0 < jitter_p, then b = 1 + (2 u1 - 1) B, c = 1 + (2 u2 - 1) C, sat = 1 + (2 u3 - 1) S, hue = (2 u4 - 1) Hh (else their identity
    values); gray = u5 < gray_p; blur on iff u6 < blur_p, with sigma = lo + u7 (hi - lo)"""
    u = [float(v) for v in rng.random(8)]
    (B, C, S, Hh), (lo, hi) = (float(v) for v in jitter), (float(v) for v in sigma)
    b, c, sat, hue = IDENTITY_PHOTOMETRIC[:4]
    if u[0] < jitter_p:
        b, c, sat, hue = 1.0 + (2.0 * u[1] - 1.0) * B, 1.0 + (2.0 * u[2] - 1.0) * C, 1.0 + (2.0 * u[3] - 1.0) * S, (2.0 * u[4] - 1.0) * Hh
    return b, c, sat, hue, 1.0 if u[5] < gray_p else 0.0, lo + u[7] * (hi - lo) if u[6] < blur_p else 0.0


def step_photometric(n: int, seed: int, rank: int, it: int, per: str = "sample", jitter=(0.5, 0.5, 0.5, 0.25), jitter_p: float = 0.8,
                     gray_p: float = 0.2, blur_p: float = 0.5, sigma=(0.1, 2.0)) -> List[PhotometricRow]:
    """the n parameter rows of one training step as a pure function of (seed, rank, iteration): `per` "sample" = one draw per sample in
    sample order, "batch" = one draw for all samples.  The generator is np.random.default_rng([seed, rank, it, 2]): a key neither
    `step_generators` (three elements) nor `step_transforms` (key 1) uses, so a step's boxes and transforms do not depend on this
    option; eight uniforms per draw (`draw_photometric`), so one sample's outcome never shifts another's."""
    if per not in ("batch", "sample"):
        raise ValueError(f"hard_aug_per must be 'batch' or 'sample', got {per!r}")
    check_photometric_ranges(jitter, jitter_p, gray_p, blur_p, sigma)
    rng = np.random.default_rng([int(seed), int(rank), int(it), 2])
    if per == "batch":
        return [draw_photometric(rng, jitter, jitter_p, gray_p, blur_p, sigma)] * int(n)
    return [draw_photometric(rng, jitter, jitter_p, gray_p, blur_p, sigma) for _ in range(int(n))]


def _gray(r, g, b):
    return 0.299 * r + 0.587 * g + 0.114 * b


def _hue_torch(r, g, b, hue: float):
    """step 4 of the definition on float32 planes"""
    mx, mn = torch.maximum(r, torch.maximum(g, b)), torch.minimum(r, torch.minimum(g, b))
    v, cr = mx, mx - mn
    flat = cr == 0
    s = torch.where(flat, torch.zeros_like(cr), cr / torch.where(flat, torch.ones_like(mx), mx))
    d = torch.where(flat, torch.ones_like(cr), cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    h6 = torch.where(mx == r, bc - gc, torch.where(mx == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = h6 / 6.0 + 1.0
    h = h - torch.floor(h)
    h = h + hue
    h = h - torch.floor(h)
    fi = torch.floor(6.0 * h)
    f = 6.0 * h - fi
    i = fi.long() % 6
    p_, q, t = (v * (1.0 - s)).clamp(0.0, 1.0), (v * (1.0 - f * s)).clamp(0.0, 1.0), (v * (1.0 - (1.0 - f) * s)).clamp(0.0, 1.0)
    pick = lambda opts: torch.stack(opts).gather(0, i[None])[0]
    return pick([v, q, p_, p_, t, v]), pick([t, v, v, q, p_, p_]), pick([p_, p_, t, v, v, q])


def _blur_torch(x: torch.Tensor, taps: np.ndarray, r: int) -> torch.Tensor:
    """step 6 on (3, h, w) float32 planes: rows, then columns, reflect-101; the kernel's order of addition (pairs, outermost first)"""
    pad = torch.nn.functional.pad
    for dim in (2, 1):
        padded = pad(x[None], (r, r, 0, 0) if dim == 2 else (0, 0, r, r), mode="reflect")[0]
        n = x.shape[dim]
        acc = torch.zeros_like(x)
        for k in range(r, 0, -1):
            acc = acc + float(taps[k]) * (padded.narrow(dim, r - k, n) + padded.narrow(dim, r + k, n))
        x = acc + float(taps[0]) * padded.narrow(dim, r, n)
    return x


def _photometric_torch(t: torch.Tensor, rows: np.ndarray, radii: np.ndarray, taps: np.ndarray) -> torch.Tensor:
    """the definition (include/vqseg.h: vqseg_photometric_f) with float32 torch ops, sample by sample: CPU tensors"""
    out = torch.empty_like(t)
    one = np.float32(1.0)
    for s in range(t.shape[0]):
        b, c, sat, hue, gray, _sigma = rows[s]              # float32 scalars: (1 - c) below is a float32 difference
        r_ = int(radii[s])
        if (b, c, sat, hue, gray, r_) == (1.0, 1.0, 1.0, 0.0, 0.0, 0):
            out[s] = t[s]                                    # by bits
            continue
        r, g, bl = t[s, 0], t[s, 1], t[s, 2]
        if b != 1.0:
            r, g, bl = ((float(b) * p).clamp(0.0, 1.0) for p in (r, g, bl))
        if c != 1.0:
            o = float(one - c) * _gray(r, g, bl).mean()
            r, g, bl = ((float(c) * p + o).clamp(0.0, 1.0) for p in (r, g, bl))
        if sat != 1.0:
            o = float(one - sat) * _gray(r, g, bl)
            r, g, bl = ((float(sat) * p + o).clamp(0.0, 1.0) for p in (r, g, bl))
        if hue != 0.0:
            r, g, bl = _hue_torch(r, g, bl, float(hue))
        if gray != 0.0:
            r = g = bl = _gray(r, g, bl)
        x = torch.stack([r, g, bl])
        out[s] = _blur_torch(x, taps[s], r_) if r_ else x
    return out


def photometric(t: torch.Tensor, params) -> torch.Tensor:
    """out[s] = t[s] through the photometric ops of params[s] = (b, c, sat, hue, gray, sigma) -- brightness, contrast, saturation, hue,
    grayscale, Gaussian blur, in this order, identity values skipped (the definition: include/vqseg.h, vqseg_photometric_f; an
    all-identity row returns the sample's bits).  t: (n, 3, H, W) float32 RGB in [0, 1], NCHW or channels_last; a new tensor of the
    same layout.  On the GPU: the photometric kernel (a mean pass when a contrast is on, then one launch); CPU tensors: the same
    definition with float32 torch ops.  ValueError: a tensor that is not (n, 3, H, W) float32, a row count other than n, |hue| > 0.5,
    a sigma whose radius ceil(3 sigma) is above 8 or above min(H, W) - 1."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
        raise ValueError("photometric: a (n, 3, H, W) tensor of RGB planes required")
    if t.dtype != torch.float32:
        raise ValueError(f"photometric: a float32 tensor required, got {t.dtype}")
    if t.is_cuda:
        return _hip.photometric(_dense(t), params)
    rows, radii, taps = _hip.photometric_rows(params, t.shape[0], t.shape[2], t.shape[3])
    return _photometric_torch(t, rows, radii, taps)


class StrongPhotometric:
    """The strong view of weak-to-strong consistency training as a callable, for use outside the trainer: `__call__(batch) -> batch'`
    draws one row per sample (`per` "sample") or one for the batch ("batch") with `draw_photometric` from this object's OWN
    np.random.Generator (`seed`; None = fresh entropy) -- nothing is taken from the global generators -- and applies `photometric`.
    `last_params`: the rows of the last call."""

    def __init__(self, brightness: float = 0.5, contrast: float = 0.5, saturation: float = 0.5, hue: float = 0.25, jitter_p: float = 0.8,
                 gray_p: float = 0.2, blur_p: float = 0.5, sigma=(0.1, 2.0), per: str = "sample", seed: Optional[int] = None):
        if per not in ("batch", "sample"):
            raise ValueError(f"per must be 'batch' or 'sample', got {per!r}")
        self.draw = dict(jitter=(brightness, contrast, saturation, hue), jitter_p=jitter_p, gray_p=gray_p, blur_p=blur_p, sigma=tuple(sigma))
        check_photometric_ranges(**self.draw)
        self.per = per
        self.rng = np.random.default_rng(seed)
        self.last_params: List[PhotometricRow] = []

    def __call__(self, batch: torch.Tensor) -> torch.Tensor:
        n = batch.shape[0]
        self.last_params = [draw_photometric(self.rng, **self.draw)] * n if self.per == "batch" else \
            [draw_photometric(self.rng, **self.draw) for _ in range(n)]
        return photometric(batch, self.last_params)


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
