"""Shared by the tiled-prediction tests (vqseg_extract_windows_f, vqseg_merge_argmax_f, nnf.extract_windows / merge_argmax,
Predictor(window=...)): the cases, the input makers (tests/predict_cases.py's) and the restatement of the merge with plain torch
ops, written out here on its own (it does not call the package):

    starts[k] = min(k * stride, extent - window),  k = 0 .. ceil((extent - window) / stride)
    per view:  acc = sum over the windows, rows then columns ascending, of w * resize(window logits un-flipped, window)   (zero elsewhere)
               ws  = the same sum of w;   m = acc / ws
    z = (m_0 + m_1 + ...) * (1 / V if V > 1);   label = z.argmax(1);   top = softmax(z, 1).max(1);   counts as predict_cases.confusion
    w = 1 ("uniform") or min(r + 1, window - r) along each axis, multiplied ("linear")

Cases: the smallest at which the kernel can still go wrong -- a clamped last window (three windows deep on an axis at stride =
window / 2), disjoint windows, up- and down-scaled window logits, a row one pixel past a wave's 256-pixel run, many windows across,
and more than nn_grid_cap = 256 tiles (the grid-stride loop)."""
import collections
import functools

import torch
import torch.nn.functional as F

from tests import predict_cases as P

# images, classes, the size of a window's logits; window, stride, output
Case = collections.namedtuple("Case", "b c lh lw window stride size")

CASES = [
    Case(2, 3, 8, 8, (8, 8), (4, 4), (13, 19)),              # clamped last window, three deep on an axis
    Case(2, 3, 8, 8, (8, 8), (8, 8), (16, 24)),              # disjoint
    Case(1, 2, 5, 7, (10, 14), (7, 9), (23, 33)),            # up-scaled windows
    Case(2, 4, 12, 16, (6, 8), (3, 5), (9, 17)),             # down-scaled windows
    Case(3, 3, 6, 6, (9, 11), (5, 6), (9, 257)),             # one window deep in y; 257-pixel rows; 42 windows across
    Case(1, 3, 16, 16, (16, 16), (8, 8), (40, 300)),         # 4 x 37 windows
]
GRID_STRIDE = Case(3, 3, 50, 50, (100, 100), (50, 50), (300, 300))      # 3 x 88 = 264 tiles under nn_grid_cap = 256; exact 2 x taps
IDS = [f"{k.b}x{k.c}x{k.lh}x{k.lw}-w{k.window[0]}x{k.window[1]}-s{k.stride[0]}x{k.stride[1]}-{k.size[0]}x{k.size[1]}" for k in CASES]
BLENDS = ["uniform", "linear"]
VIEW_FLIPS = {1: [0], 2: [1, 2], 4: [0, 1, 2, 3]}


def starts(extent, window, stride):
    n = (extent - window + stride - 1) // stride + 1
    return [min(k * stride, extent - window) for k in range(n)]


def grid_of(case):
    """(ys, xs): the window starts per axis"""
    return starts(case.size[0], case.window[0], case.stride[0]), starts(case.size[1], case.window[1], case.stride[1])


def rows_of(case):
    ys, xs = grid_of(case)
    return case.b * len(ys) * len(xs)


def shape_of(case):
    """the shape of a view: (B * T, C, lh, lw)"""
    return (rows_of(case), case.c, case.lh, case.lw)


def logits(case, seed=0, kind="normal"):
    """predict_cases.logits at the case's view shape (shared: do not modify)"""
    return P.logits(shape_of(case), seed, kind)


@functools.lru_cache(maxsize=None)
def tied(case, seed=0):
    """the "ties" logits with class 1 a copy of class 0 in EVERY window of image 0: whatever the blend, the two tie at every pixel
    of image 0 (the same sums of the same numbers), and the first maximum must win"""
    z = logits(case, seed, "ties").clone()
    t = rows_of(case) // case.b
    z[:t, 1] = z[:t, 0]
    return z


def targets(case, seed=0, dtype=torch.int64):
    return P.targets((case.b, case.c, case.lh, case.lw), case.size, seed, dtype)


def weights(case, blend, dtype=torch.float32):
    wh, ww = case.window
    if blend == "uniform":
        return torch.ones((wh, ww), dtype=dtype)
    ry, rx = torch.arange(wh, dtype=dtype), torch.arange(ww, dtype=dtype)
    return torch.minimum(ry + 1, wh - ry)[:, None] * torch.minimum(rx + 1, ww - rx)[None, :]


def merged(views, flips, case, blend, dtype=None):
    """the blended mean logits (B, C, Ho, Wo) with torch ops on the views' device; `dtype` float64 for the independent reference"""
    ys, xs = grid_of(case)
    wh, ww = case.window
    z = None
    for v, f in zip(views, flips):
        v = v if dtype is None else v.to(dtype)
        v = v.flip(P.FLIP_DIMS[f]) if f else v
        s = F.interpolate(v, size=(wh, ww), mode="bilinear", align_corners=False).reshape(case.b, len(ys) * len(xs), case.c, wh, ww)
        w = weights(case, blend, s.dtype).to(s.device)
        acc = torch.zeros((case.b, case.c) + tuple(case.size), dtype=s.dtype, device=s.device)
        ws = torch.zeros(tuple(case.size), dtype=s.dtype, device=s.device)
        for j, y0 in enumerate(ys):
            for i, x0 in enumerate(xs):
                acc[:, :, y0:y0 + wh, x0:x0 + ww] += w * s[:, j * len(xs) + i]
                ws[y0:y0 + wh, x0:x0 + ww] += w
        m = acc / ws
        z = m if z is None else z + m
    return z * (1.0 / len(views)) if len(views) > 1 else z


def restatement(views, flips, case, blend, target=None, dtype=None):
    """-> (z, label int64, top, counts | None) with torch ops"""
    z = merged(views, flips, case, blend, dtype)
    label = z.argmax(dim=1)
    top = torch.softmax(z, dim=1).max(dim=1).values
    counts = P.confusion(label, target, case.c) if target is not None else None
    return z, label, top, counts


@functools.lru_cache(maxsize=None)
def reference(case, n_views, blend):
    """computed once per (case, V, blend) and shared -- do not modify:
    (z64, label64, top64, decided = fp64 top-two gap above P.GAP, own = what the fp32 restatement deviates from z64)"""
    flips = VIEW_FLIPS[n_views]
    host = [logits(case, s) for s in range(n_views)]
    z64, label64, top64, _ = restatement(host, flips, case, blend, dtype=torch.float64)
    top2 = z64.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > P.GAP
    own = (merged(host, flips, case, blend).double() - z64).abs().max().item()
    return z64, label64, top64, decided, own


def images(case, seed=0):
    """CPU float32 (b, 3, Ho, Wo) in [0, 1) (shared: do not modify)"""
    return _images(case.b, case.size, seed)


@functools.lru_cache(maxsize=None)
def _images(b, size, seed):
    return torch.rand((b, 3) + tuple(size), generator=torch.Generator().manual_seed(500 + seed + size[0] + 3 * size[1]))
