"""Connected regions of a label map: labels, the instance table, and the removal of small regions (the reference does this on the
host, per file, with skimage / cv2: measure.label, regionprops, remove_small_objects; here the maps stay on the device).

The definition is the one stated in include/vqseg.h -- a region is a maximal set of non-ignored pixels of one image with equal value,
4- or 8-connected; its root is its smallest row-major index, its id its rank among the image's regions by rising root, which is
scipy.ndimage.label's numbering minus one.  Everything is integer arithmetic, so every output is exact.

Device tensors the kernels take go to them (nnf.region_roots / region_ids / region_table / filter_regions: vqseg_region_*); CPU
tensors, numpy arrays and whatever the kernels do not take go through the torch-op form of the same definition below: the index map
is lowered to the minimum over each pixel's equal-valued neighbours, with pointer jumping in between, until nothing changes.

    ids, counts = label_regions(pred, connectivity=8, ignore=(0,))      # (B, H, W) int32 in [-1, count), (B,) int32
    plants = region_table(pred, ignore=(0,))                            # Regions(count, value, area, bbox, centroid, root)
    clean = remove_small_regions(pred, 64, fill="neighbour")            # specks take the value next to them
    labels = enforce_connectivity(slic_labels, 16)                      # superpixel maps: still valid for superpixel_mean
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import nnf
from .maps import as_map as _as_map, back as _back, shift as _shift

# count (B,) int32; value, area, root (B, capacity) int32; bbox (B, capacity, 4) int32 = (ymin, xmin, ymax, xmax), inclusive;
# centroid (B, capacity, 2) float64 = (sum y, sum x) / area.  Row `id`; rows from min(count, capacity) on are zero.
Regions = namedtuple("Regions", "count value area bbox centroid root")


def roots_torch(values: torch.Tensor, connectivity: int = 4, ignore=()) -> torch.Tensor:
    """the torch-op form of nnf.region_roots on any device: (B, H, W) int32"""
    conn, ign = nnf.region_settings(connectivity, ignore, "roots_torch")
    b, h, w = values.shape
    n = h * w
    v = values.long()
    valid = torch.ones_like(v, dtype=torch.bool)
    for i in ign:
        valid &= v != i
    steps = [(0, -1), (0, 1), (-1, 0), (1, 0)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    # joined[k]: the pixel and its neighbour in direction k belong together (both valid, equal value)
    joined = [valid & _shift(valid, dy, dx, False) & (v == _shift(v, dy, dx, 0)) for dy, dx in steps]
    own = torch.arange(n, device=v.device).view(1, h, w).expand(b, h, w)
    idx = own.clone()
    while True:
        new = idx
        for (dy, dx), j in zip(steps, joined):
            new = torch.where(j, torch.minimum(new, _shift(idx, dy, dx, n)), new)
        flat = new.reshape(b, n)
        new = flat.gather(1, flat).view(b, h, w)            # pointer jumping: an index map entry names a pixel of the same region
        if torch.equal(new, idx):
            break
        idx = new
    return torch.where(valid, idx, torch.full_like(idx, -1)).to(torch.int32)


def ids_torch(roots: torch.Tensor):
    """the torch-op form of nnf.region_ids: (ids int32 (B, H, W), counts int32 (B,))"""
    b, h, w = roots.shape
    n = h * w
    r = roots.reshape(b, n).long()
    ok = (r >= 0) & (r < n)
    rs = torch.where(ok, r, torch.zeros_like(r))
    is_root = ok & (r == torch.arange(n, device=r.device))
    rank = torch.cumsum(is_root.long(), dim=1) - 1
    member = ok & is_root.gather(1, rs)
    ids = torch.where(member, rank.gather(1, rs), torch.full_like(r, -1))
    return ids.view(b, h, w).to(torch.int32), is_root.sum(dim=1).to(torch.int32)


def areas_torch(roots: torch.Tensor) -> torch.Tensor:
    b, h, w = roots.shape
    n = h * w
    r = roots.reshape(b, n).long()
    ok = (r >= 0) & (r < n)
    out = torch.zeros((b, n), dtype=torch.int64, device=r.device)
    out.scatter_add_(1, torch.where(ok, r, torch.zeros_like(r)), ok.long())
    return out.view(b, h, w).to(torch.int32)


def table_torch(values, roots, ids, capacity: int):
    """the torch-op form of nnf.region_table: (table int32 (B, capacity, 8), moments int64 (B, capacity, 2))"""
    b, h, w = roots.shape
    n = h * w
    dev = roots.device
    r, l, v = roots.reshape(b, n).long(), ids.reshape(b, n).long(), values.reshape(b, n).long()
    ok = (r >= 0) & (r < n) & (l >= 0) & (l < capacity)
    rows = torch.where(ok, l, torch.full_like(l, capacity))             # row `capacity`: a dump for the pixels without a row
    ys = (torch.arange(n, device=dev) // w).expand(b, n)
    xs = (torch.arange(n, device=dev) % w).expand(b, n)
    big = torch.iinfo(torch.int64).max

    def fold(src, reduce, start):
        return torch.full((b, capacity + 1), start, dtype=torch.int64, device=dev).scatter_reduce_(1, rows, src, reduce)[:, :capacity]

    area = fold(ok.long(), "sum", 0)
    root = fold(r, "amin", big)
    used = area > 0
    value = v.gather(1, torch.where(used, root, torch.zeros_like(root)))
    cols = [value, area, fold(ys, "amin", big), fold(xs, "amin", big), fold(ys, "amax", -1), fold(xs, "amax", -1), root, torch.zeros_like(area)]
    table = torch.where(used[..., None], torch.stack(cols, dim=2), torch.zeros((), dtype=torch.int64, device=dev))
    moments = torch.stack([fold(ys, "sum", 0), fold(xs, "sum", 0)], dim=2)
    return table.to(torch.int32), moments


def filter_torch(values, roots, areas, min_area: int, fill):
    """the torch-op form of nnf.filter_regions' gather; fill: "neighbour" or an integer of the map's type"""
    neighbour, const = (True, 0) if isinstance(fill, str) else (False, int(fill))
    b, h, w = roots.shape
    n = h * w
    v, r, a = values.reshape(b, n), roots.reshape(b, n).long(), areas.reshape(b, n)
    ok = (r >= 0) & (r < n)
    rs = torch.where(ok, r, torch.zeros_like(r))
    small = ok & (a.gather(1, rs) < min_area)
    if not neighbour:
        return torch.where(small, torch.full_like(v, const), v).view(b, h, w)
    ry, rx = rs // w, rs % w
    own = torch.arange(n, device=r.device).expand(b, n)
    src = torch.where(rx > 0, rs - 1, torch.where(ry > 0, rs - w, own))
    return torch.where(small, v.gather(1, src), v).view(b, h, w)


def _roots(t, connectivity, ignore):
    """(roots, whether the kernels made them: the same form then makes ids and table)"""
    if nnf.regions_supported(t):
        return nnf.region_roots(t, connectivity, ignore), True
    return roots_torch(t, connectivity, ignore), False


def label_regions(values, connectivity: int = 4, ignore=()):
    """(ids, counts) of the connected regions of `values`, an integer map (B, H, W) or (H, W), tensor or numpy array: ids int32 of the
    map's shape, a region's 0-based rank among its image's regions by rising first pixel (row-major), -1 where the value is one of
    `ignore`; counts int32 (B,) (a 0-d value for an (H, W) map).  ids + 1 with ignore=(0,) is scipy.ndimage.label's result."""
    nnf.region_settings(connectivity, ignore, "label_regions")
    t, is_np, single = _as_map(values, "label_regions")
    roots, kernels = _roots(t, connectivity, ignore)
    ids, counts = nnf.region_ids(roots) if kernels else ids_torch(roots)
    return _back(ids, is_np, single), _back(counts, is_np, single)


def region_table(values, connectivity: int = 4, ignore=(), capacity: int = 1024, return_ids: bool = False) -> Regions:
    """The instance table of `values` -> Regions(count, value, area, bbox, centroid, root), row `id` of label_regions: a region's
    value, its pixel count, its inclusive bounding box (ymin, xmin, ymax, xmax), its centroid (y, x) in float64 -- the integer sums
    divided by the area -- and its first pixel's index.  `capacity` rows per image; regions beyond them are counted in `count` and
    have no row, rows beyond `count` are zero.  `return_ids`: (Regions, ids)."""
    nnf.region_settings(connectivity, ignore, "region_table")
    if isinstance(capacity, bool) or int(capacity) != capacity or int(capacity) < 1:
        raise ValueError(f"region_table: capacity must be a positive integer, got {capacity!r}")
    capacity = int(capacity)
    t, is_np, single = _as_map(values, "region_table")
    roots, kernels = _roots(t, connectivity, ignore)
    if kernels:
        ids, counts = nnf.region_ids(roots)
        table, moments = nnf.region_table(t, roots, ids, counts, capacity)
    else:
        ids, counts = ids_torch(roots)
        table, moments = table_torch(t, roots, ids, capacity)
    area = table[..., 1]
    centroid = moments.double() / area.clamp_min(1).double()[..., None]
    parts = (counts, table[..., 0], area, table[..., 2:6], centroid, table[..., 6])
    out = Regions(*(_back(p, is_np, single) for p in parts))
    return (out, _back(ids, is_np, single)) if return_ids else out


def remove_small_regions(values, min_area: int, connectivity: int = 4, ignore=(), fill="neighbour"):
    """`values` with every region of fewer than `min_area` pixels replaced, in the map's own type: fill="neighbour" gives it the input
    value of the pixel before the region's first pixel -- to its left, else above it; a region that starts at the image's first pixel
    stays -- and an integer gives it that value.  Ignored pixels keep their value.  One pass over the INPUT: what a removed region
    turns into may itself be small, or join two regions; no cascade is claimed."""
    nnf.region_settings(connectivity, ignore, "remove_small_regions")
    min_area = nnf.region_min_area(min_area, "remove_small_regions")
    t, is_np, single = _as_map(values, "remove_small_regions")
    if nnf.regions_supported(t):
        out = nnf.filter_regions(t, min_area, connectivity, ignore, fill)
    else:
        if not isinstance(fill, str):
            info = torch.iinfo(t.dtype)
            if isinstance(fill, bool) or int(fill) != fill or not info.min <= int(fill) <= info.max:
                raise ValueError(f"remove_small_regions: fill must be 'neighbour' or an integer in {info.min}..{info.max} for {t.dtype}, got {fill!r}")
        elif fill != "neighbour":
            raise ValueError(f"remove_small_regions: fill must be 'neighbour' or an integer, got {fill!r}")
        roots = roots_torch(t, connectivity, ignore)
        out = filter_torch(t, roots, areas_torch(roots), min_area, fill)
    return _back(out, is_np, single)


def enforce_connectivity(labels, min_size: int, connectivity: int = 4):
    """Superpixel maps (utils.superpixel.slic makes none that are connected): every connected piece of a label smaller than `min_size`
    pixels takes the label next to it -- remove_small_regions(labels, min_size, fill="neighbour", ignore=()).  No new label appears, so
    the result is still a valid input of superpixel_mean / nnf.segment_mean with the same segment count.  Not applied inside
    saliency_rbd, whose label maps must stay local to the grid."""
    return remove_small_regions(labels, min_size, connectivity=connectivity, ignore=(), fill="neighbour")
