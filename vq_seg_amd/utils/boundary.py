"""Boundary metrics of class maps: class contours, the exact Euclidean distance transform, boundary F1, boundary IoU and the Hausdorff
distance (the reference scores region overlap only; on the host these rest on scipy.ndimage.distance_transform_edt per image and class,
here the maps stay on the device).

The definition is the one stated in include/vqseg.h.  A pixel is a boundary pixel of class c when it has the value c and one of its
4-neighbours inside the image has another, non-ignored value; d2 is the squared distance to the nearest boundary pixel of the plane
(EDT_NONE on a plane without one); per image and class eight integers are counted -- boundary pixels of prediction and target, how
many of each lie within `tolerance` of the other's, the inner bands of width `width` of both masks and their overlap, and the largest
distance either way -- and the scores are ratios of those in float64, NaN where a denominator is zero.

Device tensors the kernels take go to them (nnf.class_boundaries / edt_sq / boundary_counts: vqseg_boundary_*); CPU tensors, numpy arrays
and whatever the kernels do not take go through the torch-op form of the same definition below: the row pass from cummax / cummin, the
column pass as a chunked minimum over the rows.  All of it is integer arithmetic, so both forms agree exactly.

    d = distance_transform(mask)                                        # float32 distances to the nearest non-zero pixel, inf without one
    stats = boundary_stats(pred, target, 3, tolerance=2.0)              # BoundaryStats(table, f1, precision, recall, iou, hausdorff)
    m = BoundaryMeasurement(3); m.update(pred, target); m.result()      # data-set means, NaN skipped
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np
import torch

from .. import nnf
from .maps import as_map as _as_map, back as _back, shift as _shift

EDT_NONE = nnf.EDT_NONE

# table (B, C, 8) int32 = (n_pred, hit_pred, n_gt, hit_gt, band_inter, band_union, hd_pred_sq, hd_gt_sq); the scores (B, C) float64 numpy
# arrays with NaN where undefined
BoundaryStats = namedtuple("BoundaryStats", "table f1 precision recall iou hausdorff")

_CHUNK = 1 << 24                                                # elements of the (planes, rows, j, W) block of the torch-op column pass


# ------------------------------------------------------------------------------------------------------------------------------
# the torch-op form
# ------------------------------------------------------------------------------------------------------------------------------
def boundaries_torch(labels: torch.Tensor, num_classes: int, ignore=()) -> torch.Tensor:
    """the torch-op form of nnf.class_boundaries on any device: (B, C, H, W) uint8"""
    v = labels.long()
    out = []
    for c in range(num_classes):
        edge = torch.zeros_like(v, dtype=torch.bool)
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            q = _shift(v, dy, dx, c)                            # outside the image: the class itself, which makes no boundary
            other = q != c
            for i in ignore:
                other &= q != int(i)
            edge |= other
        out.append((v == c) & edge)
    return torch.stack(out, dim=1).to(torch.uint8)


def edt_sq_torch(seeds: torch.Tensor) -> torch.Tensor:
    """the torch-op form of nnf.edt_sq on any device: (..., H, W) -> int32"""
    h, w = seeds.shape[-2:]
    s = (seeds != 0).reshape(-1, h, w)
    planes, dev = s.shape[0], s.device
    far = 1 << 20                                               # a column no row reaches
    x = torch.arange(w, device=dev, dtype=torch.int32).expand(planes, h, w)
    left = torch.where(s, x, torch.full_like(x, -far)).cummax(dim=2).values
    right = torch.where(s, x, torch.full_like(x, far)).flip(2).cummin(dim=2).values.flip(2)
    g = torch.minimum(x - left, right - x).clamp(max=0x7fff)    # (a row without a seed: far away; its square still fits)
    has = s.any(dim=2)                                          # (planes, H)
    y = torch.arange(h, device=dev, dtype=torch.int32)
    out = torch.empty((planes, h, w), dtype=torch.int32, device=dev)
    none = torch.full((), EDT_NONE, dtype=torch.int32, device=dev)
    pstep = max(1, _CHUNK // (h * w))
    for p0 in range(0, planes, pstep):
        gp, hp = g[p0:p0 + pstep], has[p0:p0 + pstep]
        g2 = gp * gp                                            # (p, j, W)
        ystep = max(1, _CHUNK // (gp.shape[0] * h * w))
        for y0 in range(0, h, ystep):
            dy2 = (y[y0:y0 + ystep, None] - y[None, :]) ** 2    # (rows, j)
            cand = torch.where(hp[:, None, :, None], g2[:, None] + dy2[None, :, :, None], none)       # a row without a seed offers nothing
            out[p0:p0 + pstep, y0:y0 + ystep] = cand.min(dim=2).values
    return out.view(seeds.shape)


def counts_torch(pred, target, num_classes: int, tol_sq: int, width_sq: int, ignore=()) -> torch.Tensor:
    """the torch-op form of nnf.boundary_counts on any device: (B, C, 8) int32"""
    p, t = pred.long(), target.long()
    bp, bg = boundaries_torch(p, num_classes, ignore), boundaries_torch(t, num_classes, ignore)
    dp, dg = edt_sq_torch(bp), edt_sq_torch(bg)
    valid = torch.ones_like(t, dtype=torch.bool)
    for i in ignore:
        valid &= t != int(i)
    cls = torch.arange(num_classes, device=p.device)[None, :, None, None]
    valid = valid[:, None]
    p_edge, g_edge = valid & (bp != 0), valid & (bg != 0)
    pd = valid & (p[:, None] == cls) & (dp <= width_sq)
    gd = valid & (t[:, None] == cls) & (dg <= width_sq)

    def count(m):
        return m.flatten(2).sum(dim=2)

    def farthest(d, edge, n, other):
        m = torch.where(edge, d, torch.full_like(d, -1)).flatten(2).max(dim=2).values
        return torch.where((n > 0) & other.flatten(2).any(dim=2), m, torch.full_like(m, -1))

    n_pred, n_gt = count(p_edge), count(g_edge)
    cols = [n_pred, count(p_edge & (dg <= tol_sq)), n_gt, count(g_edge & (dp <= tol_sq)), count(pd & gd), count(pd | gd),
            farthest(dg, p_edge, n_pred, bg != 0).long(), farthest(dp, g_edge, n_gt, bp != 0).long()]
    return torch.stack(cols, dim=2).to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# scores
# ------------------------------------------------------------------------------------------------------------------------------
def scores_from_table(table) -> BoundaryStats:
    """BoundaryStats of a (..., 8) count table (tensor or numpy array): float64 ratios, NaN where undefined.  F is NaN when neither map
    has a boundary pixel of the class, 0 when exactly one has none or when P + R == 0."""
    t = (table.detach().cpu().numpy() if torch.is_tensor(table) else np.asarray(table)).astype(np.float64)
    n_pred, hit_pred, n_gt, hit_gt, inter, union, hd_p, hd_g = (t[..., k] for k in range(8))
    nan = np.full(t.shape[:-1], np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = np.where(n_pred > 0, hit_pred / n_pred, nan)
        recall = np.where(n_gt > 0, hit_gt / n_gt, nan)
        both = (n_pred > 0) & (n_gt > 0)
        s = precision + recall
        f1 = np.where(both & (s > 0), 2 * precision * recall / s, np.where((n_pred > 0) | (n_gt > 0), 0.0, nan))
        iou = np.where(union > 0, inter / union, nan)
        hd = np.where((hd_p >= 0) & (hd_g >= 0), np.sqrt(np.maximum(np.maximum(hd_p, hd_g), 0)), nan)
    return BoundaryStats(table, f1, precision, recall, iou, hd)


def mean_over_classes(x):
    """(the mean, the per-class means) of a (N, C) score over all images: NaN is skipped, a class that is NaN for every image is NaN in
    the list and left out of the mean, and the mean of nothing is NaN"""
    x = np.asarray(x, dtype=np.float64)
    ok = ~np.isnan(x)
    n = ok.sum(axis=0)
    per = np.where(n > 0, np.where(ok, x, 0.0).sum(axis=0) / np.maximum(n, 1), np.nan)
    return (float(per[n > 0].mean()) if (n > 0).any() else float("nan")), per


# ------------------------------------------------------------------------------------------------------------------------------
# the public surface
# ------------------------------------------------------------------------------------------------------------------------------
def _threshold(value, name, who):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value) or value < 0 or \
            float(value) ** 2 >= EDT_NONE:
        raise ValueError(f"{who}: {name} must be a finite number >= 0 whose square fits int32, got {value!r}")
    return int(math.floor(float(value) ** 2))


def boundary_settings(num_classes, tolerance=2.0, width=None, ignore=(255,), who="boundary_stats"):
    """the checked (num_classes, tol_sq, width_sq, ignore tuple) of a boundary call; width=None means the tolerance"""
    c = nnf.boundary_classes(num_classes, who)
    tol_sq = _threshold(tolerance, "tolerance", who)
    width_sq = tol_sq if width is None else _threshold(width, "width", who)
    _conn, ign = nnf.region_settings(4, ignore, who)
    return c, tol_sq, width_sq, ign


def boundary_tolerance(h: int, w: int, ratio: float = 0.0075) -> int:
    """a size-relative tolerance, the rule of the video-segmentation benchmarks: max(1, round(ratio * the image diagonal))"""
    return max(1, int(round(ratio * math.hypot(h, w))))


def distance_transform(mask, squared: bool = False):
    """Distances to the nearest non-zero pixel of `mask` (..., H, W), uint8 or bool, tensor or numpy array, every leading dimension a batch
    of independent planes: int32 squared distances (EDT_NONE on a plane without a non-zero pixel) with squared=True, else their float32
    root (inf there).  scipy.ndimage.distance_transform_edt(mask == 0) is the same map: it measures to the nearest ZERO."""
    is_np = isinstance(mask, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(mask)) if is_np else mask
    if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.bool) or t.dim() < 2 or t.numel() == 0:
        raise ValueError(f"distance_transform: a uint8 or bool mask (..., H, W) is required, got "
                         f"{getattr(t, 'dtype', type(mask).__name__)} {tuple(getattr(t, 'shape', ()))}")
    t = t.detach()
    kernels = t.is_cuda and t.shape[-2] <= nnf.EDT_MAX_SIDE and t.shape[-1] <= nnf.EDT_MAX_SIDE
    d2 = nnf.edt_sq(t) if kernels else edt_sq_torch(t)
    out = d2 if squared else torch.where(d2 == EDT_NONE, torch.full((), math.inf, device=d2.device), d2.float().sqrt())
    return out.cpu().numpy() if is_np else out


def class_boundaries(labels, num_classes: int, ignore=(255,)):
    """(B, C, H, W) uint8 of 0 / 1 (or (C, H, W) for an (H, W) map): the boundary pixels of every class of `labels`, an integer map, tensor
    or numpy array -- the pixels of the class with a 4-neighbour inside the image of another, non-ignored value"""
    c, _t, _w, ign = boundary_settings(num_classes, ignore=ignore, who="class_boundaries")
    t, is_np, single = _as_map(labels, "class_boundaries")
    out = nnf.class_boundaries(t, c, ign) if nnf.boundaries_supported(t) and t.shape[0] * c <= nnf.EDT_MAX_PLANES else boundaries_torch(t, c, ign)
    return _back(out, is_np, single)


def boundary_table(pred, target, num_classes: int, tol_sq: int, width_sq: int, ignore=()):
    """the (B, C, 8) int32 count table as a tensor on the maps' device, by the kernels where they take the maps"""
    p, _np, _single = _as_map(pred, "boundary_stats")
    t, _np, _single = _as_map(target, "boundary_stats")
    if tuple(p.shape) != tuple(t.shape):
        raise ValueError(f"boundary_stats: pred and target must have one shape, got {tuple(p.shape)} and {tuple(t.shape)}")
    if p.device != t.device:
        t = t.to(p.device)
    if nnf.boundaries_supported(p) and nnf.boundaries_supported(t):
        return nnf.boundary_counts(p, t, num_classes, tol_sq, width_sq, ignore)
    return counts_torch(p, t, num_classes, tol_sq, width_sq, ignore)


def boundary_stats(pred, target, num_classes: int, tolerance: float = 2.0, width=None, ignore=(255,)) -> BoundaryStats:
    """BoundaryStats(table, f1, precision, recall, iou, hausdorff) of the class maps `pred` and `target`, integer maps (B, H, W) or (H, W),
    tensors or numpy arrays.  table: the (B, C, 8) int32 counts of include/vqseg.h, of the type and on the device it was given; the
    scores: (B, C) float64 numpy arrays, NaN where undefined.  tolerance: how far (pixels, Euclidean) a boundary pixel may lie from the
    other map's boundary and still count as a hit; width: the width of the inner band of boundary IoU (None: the tolerance).  Pixels
    whose target is one of `ignore` are not counted and make no boundary."""
    c, tol_sq, width_sq, ign = boundary_settings(num_classes, tolerance, width, ignore)
    is_np = isinstance(pred, np.ndarray)
    single = getattr(pred, "ndim", 3) == 2
    table = boundary_table(pred, target, c, tol_sq, width_sq, ign)
    s = scores_from_table(table)
    pick = (lambda a: a[0]) if single else (lambda a: a)
    return BoundaryStats(_back(table, is_np, single), *(pick(a) for a in s[1:]))


def boundary_f1(pred, target, num_classes: int, tolerance: float = 2.0, ignore=(255,)):
    return boundary_stats(pred, target, num_classes, tolerance, None, ignore).f1


def boundary_iou(pred, target, num_classes: int, width: float = 2.0, ignore=(255,)):
    return boundary_stats(pred, target, num_classes, width, width, ignore).iou


def hausdorff_distance(pred, target, num_classes: int, ignore=(255,)):
    return boundary_stats(pred, target, num_classes, 0.0, 0.0, ignore).hausdorff


class BoundaryMeasurement:
    """Data-set-level boundary scores: .update(pred_labels, target) once per batch (class maps (B, H, W), tensors or numpy arrays; only
    the (B, C, 8) table leaves the device), .result() the means over all images seen -- NaN skipped, a class that is undefined for every
    image left out of the class mean:

        boundary_f1, boundary_iou, hausdorff         floats (NaN when nothing is defined)
        boundary_f1s, boundary_ious, hausdorffs      per-class float64 arrays
        images                                       how many images were seen
    """

    def __init__(self, num_classes: int, tolerance: float = 2.0, width=None, ignore=(255,)):
        self.num_classes, self.tol_sq, self.width_sq, self.ignore = boundary_settings(num_classes, tolerance, width, ignore, "BoundaryMeasurement")
        self.tables = []

    def update(self, pred_labels, target) -> None:
        table = boundary_table(pred_labels, target, self.num_classes, self.tol_sq, self.width_sq, self.ignore)
        self.tables.append(table.detach().cpu().numpy())

    def table(self) -> np.ndarray:
        return np.concatenate(self.tables) if self.tables else np.zeros((0, self.num_classes, 8), dtype=np.int32)

    def result(self) -> dict:
        s = scores_from_table(self.table())
        out = dict(images=int(s.f1.shape[0]))
        for key, x in (("boundary_f1", s.f1), ("boundary_iou", s.iou), ("hausdorff", s.hausdorff)):
            out[key], out[key + "s"] = mean_over_classes(x)
        return out
