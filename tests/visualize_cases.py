"""Shared by the visualisation tests (vqseg_render_sheet_u8, nnf.render_sheet, vq_seg_amd.utils.visualize): shapes, input makers and the
fp64 restatement of the sheet, written out here on its own in numpy (it does not call the package):

    image    bilinear, align_corners=False, taps per ATen: s = max((d + 0.5) in / out - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, in - 1)
    target   nearest per ATen: src = min(int(dst * float32(in / out)), in - 1)
    rows     TARGET t in [0, C) else 2 C;  PRED p < C else 2 C;  DETAIL p >= C: 2 C, else p + C [p != t]
    mix      clip((1 - alpha) image + alpha palette[row], 0, 1)
    box2     mean of the 2 x 2 float colours, then quantised
    byte     floor(clip(x, 0, 1) * 255), NaN -> 0

The rule every comparison follows (`check`): palette-row pixels -- without box2 every TARGET / PRED / DETAIL / FILL pixel, with box2 those
whose four sheet pixels share one row -- equal the oracle's bytes exactly.  Elsewhere a byte may differ by one level only where the
oracle's pre-floor value lies within NEAR = 1e-3 of an integer: the f32 error of tap mix + blend + mean + x 255 is a few ulp of a value
<= 255, about 2e-4, and 1e-3 is that bound with margin.  A saturated value (NaN, or outside [0, 1] by more than NEAR / 255) is not
"near": its byte is 0 or 255 in any arithmetic and must be equal.  The share of near-integer values in a panel is a condition on the
inputs (<= 1 %; uniform float32 images give about 0.2 %), asserted so that the tolerance cannot hide a wrong panel."""
import functools

import numpy as np
import torch

KINDS = ["image", "target", "pred", "detail", "mix_pred", "mix_detail", "fill"]
NEAR = 1e-3
MAX_NEAR_SHARE = 0.01
B = 2
# (h, w) of the image -> (Ho, Wo) of the display
SHAPES = [
    ((6, 10), (12, 20)),          # Wo < 64: a wave covers several sheet rows; even sizes: box2
    ((7, 9), (33, 70)),           # odd sizes, a partial last group of 4 pixels, Wo >= 64
    ((16, 64), (16, 64)),         # identity
]
IDS = ["x".join(map(str, s)) + "-" + "x".join(map(str, o)) for s, o in SHAPES]
TARGET_OWN = (5, 7)               # a target at its own size: nearest neighbour
GAP = 20
FIVE = ["image", "target", "pred", ("fill", GAP), "mix_pred"]

_CLASS = [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
_WRONG = [[0.5, 0.5, 0.5], [230 / 255, 145 / 255, 56 / 255], [1.0, 217 / 255, 102 / 255], [0.6, 0.9, 0.6]]


def palette(c):
    """(2 C + 1, 3) float64, stated here again: class colours, "wrong" colours, white for ignore"""
    return np.array(_CLASS[:c] + _WRONG[:c] + [[1.0, 1.0, 1.0]], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def sources(c, src, size, target_size=None, special=False, seed=0):
    """CPU tensors (image (B, 3, h, w) f32 uniform in [0, 1), pred (B, Ho, Wo) u8, target (B, Ht, Wt) i64); `special`: a NaN and a value
    above 1 in the image, 255 among the targets, a pred byte >= C.  Shared: do not modify."""
    g = torch.Generator().manual_seed(4000 + 100 * seed + 10 * c + sum(src) + 3 * sum(size))
    image = torch.rand((B, 3) + tuple(src), generator=g)
    pred = torch.randint(0, c, (B,) + tuple(size), generator=g).to(torch.uint8)
    target = torch.randint(0, c, (B,) + tuple(target_size or size), generator=g)
    if special:
        image[0, 1, src[0] // 2, src[1] // 2] = float("nan")
        image[1, 2, 0, src[1] - 1] = 1.7
        target[torch.rand(target.shape, generator=g) < 0.1] = 255
        target[1, 0, 0] = -3
        pred[0, size[0] - 1, size[1] - 1] = c
        pred[1, 0, 1] = 200
    return image, pred, target


def layout(panels, wo):
    rows, x = [], 0
    for p in panels:
        kind, width = (p, wo) if isinstance(p, str) else p
        rows.append((kind, x, width))
        x += width
    return rows, x


def _taps(out, size):
    s = np.maximum((np.arange(out, dtype=np.float64) + 0.5) * (size / out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    return i0, i1, s - i0


def bilinear64(image, size):
    x = np.asarray(image, dtype=np.float64)
    h0, h1, lh = _taps(size[0], x.shape[2])
    w0, w1, lw = _taps(size[1], x.shape[3])
    lh, lw = lh[None, None, :, None], lw[None, None, None, :]
    top = (1 - lw) * x[:, :, h0][:, :, :, w0] + lw * x[:, :, h0][:, :, :, w1]
    bot = (1 - lw) * x[:, :, h1][:, :, :, w0] + lw * x[:, :, h1][:, :, :, w1]
    return (1 - lh) * top + lh * bot


def nearest(target, size):
    t = np.asarray(target)
    ht, wt = t.shape[-2:]
    ys = np.minimum((np.arange(size[0], dtype=np.float32) * (np.float32(ht) / np.float32(size[0]))).astype(np.int64), ht - 1)
    xs = np.minimum((np.arange(size[1], dtype=np.float32) * (np.float32(wt) / np.float32(size[1]))).astype(np.int64), wt - 1)
    return t[:, ys][:, :, xs]


def oracle(panels, size, c, image=None, pred=None, target=None, pal=None, fill=(1.0, 1.0, 1.0), alpha=0.4, box2=False):
    """-> (value (rows, cols, 3) float64: the colour before clip and x 255, NaN where a NaN reaches it;  exact (rows, cols) bool: the pixel
    is a palette row, its byte must be equal).  rows / cols of the canvas (halved with box2)."""
    pal = palette(c) if pal is None else np.asarray(pal, dtype=np.float64)
    ho, wo = size
    img = tgt = p = None
    if image is not None:
        img = bilinear64(image, size).transpose(0, 2, 3, 1).reshape(-1, wo, 3)
    if pred is not None:
        p = np.asarray(pred).astype(np.int64).reshape(-1, wo)
    if target is not None:
        tgt = nearest(target, size).astype(np.int64).reshape(-1, wo)
    rows = B * ho
    lay, cols = layout(panels, wo)
    value = np.zeros((rows, cols, 3))
    row_of = np.full((rows, cols), -1, dtype=np.int64)
    for kind, x0, width in lay:
        sl = slice(x0, x0 + width)
        if kind == "fill":
            value[:, sl] = np.asarray(fill, dtype=np.float64)
            row_of[:, sl] = 2 * c + 1
            continue
        if kind == "image":
            value[:, sl] = img
            continue
        if kind == "target":
            r = np.where((tgt >= 0) & (tgt < c), tgt, 2 * c)
        elif kind in ("pred", "mix_pred"):
            r = np.where(p < c, p, 2 * c)
        else:
            r = np.where(p >= c, 2 * c, np.where(p != tgt, p + c, p))
        if kind.startswith("mix"):
            with np.errstate(invalid="ignore"):
                value[:, sl] = np.clip((1 - alpha) * img + alpha * pal[r], 0, 1)          # np.clip keeps a NaN
        else:
            value[:, sl] = pal[r]
            row_of[:, sl] = r
    exact = row_of >= 0
    if box2:
        value = (value[0::2, 0::2] + value[0::2, 1::2] + value[1::2, 0::2] + value[1::2, 1::2]) / 4
        a, b_, c_, d = row_of[0::2, 0::2], row_of[0::2, 1::2], row_of[1::2, 0::2], row_of[1::2, 1::2]
        exact = (a >= 0) & (a == b_) & (a == c_) & (a == d)
    return value, exact


def to_bytes(value):
    """floor(clip(x, 0, 1) * 255), NaN -> 0"""
    return np.floor(np.clip(np.nan_to_num(value, nan=0.0), 0, 1) * 255).astype(np.uint8)


def near_integer(value):
    """where a one-level difference is admitted: a finite, unsaturated value whose pre-floor value is within NEAR of an integer"""
    v = value * 255
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v > -NEAR) & (v < 255 + NEAR) & (np.abs(v - np.round(v)) <= NEAR)


def check(got, value, exact, what, panels=None, wo=None, scale=1):
    """`got` (rows, cols, 3) uint8 against the oracle under the rule of this module's header; with `panels` the near-integer share of
    every non-exact panel is asserted as well (`scale` 2 for a box2 canvas)"""
    got = np.asarray(got)
    want = to_bytes(value)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    diff = got.astype(np.int64) - want.astype(np.int64)
    wrong_exact = (diff != 0) & exact[..., None]
    assert not wrong_exact.any(), (what, "palette-row bytes differ", int(wrong_exact.sum()), np.argwhere(wrong_exact)[:5].tolist())
    near = near_integer(value) & ~exact[..., None]
    bad = (diff != 0) & ~(near & (np.abs(diff) == 1))
    assert not bad.any(), (what, int(bad.sum()), [(idx.tolist(), int(got[tuple(idx)]), float(value[tuple(idx)] * 255)) for idx in np.argwhere(bad)[:5]])
    if panels is not None:
        for kind, x0, width in layout(panels, wo)[0]:
            if kind in ("image", "mix_pred", "mix_detail"):
                share = near[:, x0 // scale:(x0 + width) // scale].mean()
                assert share <= MAX_NEAR_SHARE, (what, kind, "near-integer share of the inputs", float(share))
    return int((diff != 0).sum())
