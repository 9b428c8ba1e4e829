"""Shared by the affine-warp / similarity-transform tests: a numpy float64 restatement of the warp (vqseg_affine_warp_f; coordinates
and weights in float64 from the FLOAT32 matrix the kernel receives), the shapes, the angles and the tolerance."""
import numpy as np

ARG_BLOCK = 64                                               # samples per launch of the kernel (its argument block)
# (n, P, h, w): single row / single column; no tile multiple, non-square, half-integer centre; two or more tiles each way with
# bf16-vectorisable channels; one sample more than an argument block holds (the multi-launch path)
SHAPES = [(2, 3, 5, 7), (1, 1, 1, 9), (1, 1, 9, 1), (2, 3, 17, 19), (3, 3, 33, 20), (2, 8, 40, 36), (ARG_BLOCK + 1, 1, 4, 4)]
SQUARE = [(2, 3, 19, 19), (ARG_BLOCK + 1, 1, 4, 4)]          # where a quarter turn is a permutation of the pixels
LABELS_3D = (2, 17, 19)
ANGLES = [17.3, -33.7, 89.99, 123.4, 0.001]                  # no 45 degrees: it puts 3-12 % of the pixels on a rounding boundary


def matrices(angle, flip, n, inverse=False):
    """rotation by `angle` degrees after no flip (code 3) / a horizontal one (5) / a vertical one (7): float32 (n, 6)"""
    from vq_seg_amd.data.augmentations import similarity_matrices
    return similarity_matrices([{None: 3, "h": 5, "v": 7}[flip]] * n, [angle] * n, inverse=inverse)


def coords(mats, h, w):
    """float64 source coordinates (xs, ys), each (n, h, w), from float32 matrices (n, 6)"""
    m = np.asarray(mats, dtype=np.float32).astype(np.float64)
    dx = (np.arange(w, dtype=np.float64) - (w - 1) / 2.0)[None, None, :]
    dy = (np.arange(h, dtype=np.float64) - (h - 1) / 2.0)[None, :, None]
    k = [m[:, i, None, None] for i in range(6)]
    return (k[0] * dx + k[1] * dy) + (w - 1) / 2.0, (k[3] * dx + k[4] * dy) + (h - 1) / 2.0


def _taps(src, xi, yi):
    """src (n, P, h, w) at integer (xi, yi) (n, h, w) -> values (n, P, h, w) and the inside mask (n, 1, h, w)"""
    n, p, h, w = src.shape
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    at = (np.clip(yi, 0, h - 1) * w + np.clip(xi, 0, w - 1)).reshape(n, 1, h * w)
    v = np.take_along_axis(src.reshape(n, p, h * w), np.broadcast_to(at, (n, p, h * w)), axis=2).reshape(n, p, h, w)
    return v, inside[:, None]


def bilinear(src, mats):
    """float64 (n, P, h, w): four taps, zero padding; a tap of weight zero is left out"""
    src = np.asarray(src, dtype=np.float64)
    h, w = src.shape[-2:]
    xs, ys = coords(mats, h, w)
    x0, y0 = np.floor(xs), np.floor(ys)
    fx, fy = (xs - x0)[:, None], (ys - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = np.zeros(src.shape, dtype=np.float64)
    for wgt, xi, yi in (((1 - fy) * (1 - fx), x0, y0), ((1 - fy) * fx, x0 + 1, y0), (fy * (1 - fx), x0, y0 + 1), (fy * fx, x0 + 1, y0 + 1)):
        v, inside = _taps(src, xi, yi)
        out += np.where(inside & (wgt != 0), wgt * v, 0.0)
    return out


def nearest(src, mats, fill):
    """-> (out, decided): the source pixel (rint(xs), rint(ys)) or `fill` outside; `decided` (n, 1, h, w) is False where xs + 0.5 or
    ys + 0.5 lies within 1e-3 of an integer: there a float32 coordinate may round to the other pixel, and nothing is compared"""
    src = np.asarray(src)
    h, w = src.shape[-2:]
    xs, ys = coords(mats, h, w)
    v, inside = _taps(src, np.rint(xs).astype(np.int64), np.rint(ys).astype(np.int64))
    decided = (np.abs(xs + 0.5 - np.rint(xs + 0.5)) > 1e-3) & (np.abs(ys + 0.5 - np.rint(ys + 0.5)) > 1e-3)
    return np.where(inside, v, np.asarray(fill, dtype=src.dtype)), decided[:, None]


def tol_f32(src, h, w):
    """8 * 2^-24 * max(h, w) * (max - min of the input): the float32 rounding of a source coordinate (a few ulp of a number below
    max(h, w)) times the steepest slope a bilinear surface over the input can have; + 8 * 2^-24 * max|input|: the rounding of the
    weights and of the four-term sum"""
    src = np.asarray(src, dtype=np.float64)
    return 8 * 2.0 ** -24 * max(h, w) * float(src.max() - src.min()) + 8 * 2.0 ** -24 * float(np.abs(src).max())


def tol_bf16(src, h, w, value):
    """the float32 bound plus one bfloat16 rounding of the result"""
    return tol_f32(src, h, w) + 2.0 ** -8 * np.abs(value)
