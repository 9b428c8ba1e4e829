"""Panoptic quality of class maps: how many objects were found, invented and missed, and how well the found ones are outlined (the
reference scores pixels only; Kirillov et al., "Panoptic Segmentation", CVPR 2019, is the public definition followed here).

The definition is the one stated in include/vqseg.h -- the connected regions (utils.regions) of the thing classes in the prediction and
in the ground truth, a one-to-one matching of regions of equal class at IoU > 0.5 with void pixels trimmed from the union, and per
image and class the counts (tp, fp, fn, n_pred, n_gt) and the float64 sum of the matched IoUs.  Counts are summed over the images of a
data set before PQ = SQ * RQ is formed.  Every table is integer and exact; iou_sum is added in a fixed order.

Device maps the kernels take go to them (nnf.region_* for ids and tables, nnf.instance_overlap / instance_tally: vqseg_instance_*);
CPU tensors, numpy arrays and whatever the kernels do not take go through the torch-op form of the same definition below: pair keys
gt_id * capacity + pred_id and torch.unique, every pair tested, no majority shortcut.

    m = match_regions(pred, target, num_classes=3)                      # InstanceMatch: both Regions, match, inter, union, void, ..
    s = panoptic_stats(pred, target, 3, void=(255,), connectivity=8)    # PanopticStats(table, iou_sum, overflow, pq, sq, rq, count_error)
    pq = panoptic_quality(pred, target, 3)
    meas = InstanceMeasurement(3); meas.update(pred, target); meas.result()["pq"]
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from .. import nnf
from .maps import as_map as _as_map, back as _back
from .regions import Regions, ids_torch, roots_torch, table_torch

# pred, target: Regions of the two sides (rows per image: capacity); match, inter, union (B, capacity) int32 by ground-truth row;
# void, matched (B, capacity) int32 by prediction row; overflow (B,) int32
InstanceMatch = namedtuple("InstanceMatch", "pred target match inter union void matched overflow")
# table (B, C, 5) int32 = (tp, fp, fn, n_pred, n_gt); iou_sum (B, C) float64; overflow (B,) int32; pq, sq, rq, count_error floats of
# the counts summed over the B images
PanopticStats = namedtuple("PanopticStats", "table iou_sum overflow pq sq rq count_error")


def _things_only(t, things, wide):
    """the map with every value that is not a thing class replaced by ONE value region_roots ignores: (map, that value).  uint8 maps
    keep their type (255 is no class: num_classes <= 255); the others, and all maps of the torch-op form, carry -1."""
    keep = torch.zeros_like(t, dtype=torch.bool)
    for c in things:
        keep |= t == c
    if t.dtype == torch.uint8 and not wide:
        return torch.where(keep, t, torch.full_like(t, 255)), 255
    t = t.to(torch.int64 if wide else t.dtype)
    return torch.where(keep, t, torch.full_like(t, -1)), -1


def _regions_of(table, moments, counts):
    area = table[..., 1]
    centroid = moments.double() / area.clamp_min(1).double()[..., None]
    return Regions(counts, table[..., 0], area, table[..., 2:6], centroid, table[..., 6])


def overlap_torch(pred_ids, gt_ids, target, pred_table, gt_table, pred_counts, gt_counts, void, capacity: int, num_classes: int):
    """the torch-op form of nnf.instance_overlap + nnf.instance_tally on any device -> nnf.InstanceTally and void_count: every pair
    (g, p) that shares a pixel is tested"""
    b, h, w = pred_ids.shape
    n, dev = h * w, pred_ids.device
    p, g, t = pred_ids.reshape(b, n).long(), gt_ids.reshape(b, n).long(), target.reshape(b, n).long()
    pok, gok = (p >= 0) & (p < capacity), (g >= 0) & (g < capacity)
    is_void = torch.zeros_like(pok)
    for v in void:
        is_void |= t == v
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    void_count = zeros(b, capacity)
    match, inter, union, matched = torch.full((b, capacity), -1, dtype=torch.int64, device=dev), zeros(b, capacity), zeros(b, capacity), zeros(b, capacity)
    overflow = ((pred_counts.long() > capacity) | (gt_counts.long() > capacity)).to(torch.int32)
    for k in range(b):
        at = pok[k] & ~gok[k] & is_void[k]
        void_count[k] = torch.bincount(p[k][at], minlength=capacity)
        if int(overflow[k]):
            continue
        both = pok[k] & gok[k]
        keys, cnt = torch.unique(g[k][both] * capacity + p[k][both], return_counts=True)
        gg, pp = keys // capacity, keys % capacity
        rows_ok = (gg < gt_counts[k].long().clamp(0, capacity)) & (pp < pred_counts[k].long().clamp(0, capacity))
        pa, ga = pred_table[k, :, 1].long(), gt_table[k, :, 1].long()
        un = pa[pp] - void_count[k][pp] + ga[gg] - cnt
        ok = rows_ok & (pred_table[k, :, 0].long()[pp] == gt_table[k, :, 0].long()[gg]) & (2 * cnt > un)
        match[k][gg[ok]], inter[k][gg[ok]], union[k][gg[ok]] = pp[ok], cnt[ok], un[ok]
        matched[k][pp[ok]] = 1
    # the tally on the host: the tables are small, and iou_sum is a sum in a fixed order
    tally = np.zeros((b, num_classes, 5), dtype=np.int32)
    iou_sum = np.zeros((b, num_classes), dtype=np.float64)
    m_, i_, u_, d_, v_ = (x.cpu().numpy() for x in (match, inter, union, matched, void_count))
    pt, gt, pc, gc, ov = (x.cpu().numpy() for x in (pred_table, gt_table, pred_counts, gt_counts, overflow))
    count = lambda classes: np.bincount(classes, minlength=num_classes)
    for k in range(b):
        if ov[k]:
            continue
        n_g, n_p = min(max(int(gc[k]), 0), capacity), min(max(int(pc[k]), 0), capacity)
        c = gt[k, :n_g, 0].astype(np.int64)
        known, hit = (c >= 0) & (c < num_classes), m_[k, :n_g] >= 0
        tally[k, :, 4], tally[k, :, 0], tally[k, :, 2] = count(c[known]), count(c[known & hit]), count(c[known & ~hit])
        sel = known & hit & (u_[k, :n_g] > 0)
        np.add.at(iou_sum[k], c[sel], i_[k, :n_g][sel].astype(np.float64) / u_[k, :n_g][sel].astype(np.float64))     # unbuffered: in rising id
        c = pt[k, :n_p, 0].astype(np.int64)
        known = (c >= 0) & (c < num_classes)
        tally[k, :, 3] = count(c[known])
        tally[k, :, 1] = count(c[known & (d_[k, :n_p] == 0) & (2 * v_[k, :n_p] <= pt[k, :n_p, 1].astype(np.int64))])
    i32 = lambda x: x.to(torch.int32)
    out = nnf.InstanceTally(i32(match), i32(inter), i32(union), i32(matched), torch.from_numpy(tally).to(dev), torch.from_numpy(iou_sum).to(dev), overflow)
    return out, i32(void_count)


def _run(pred, target, num_classes, things, void, connectivity, capacity, who):
    c, things, void, conn, capacity = nnf.instance_settings(num_classes, things, void, connectivity, capacity, who)
    p, p_np, p_single = _as_map(pred, who)
    t, t_np, t_single = _as_map(target, who)
    if tuple(p.shape) != tuple(t.shape):
        raise ValueError(f"{who}: pred and target must have one shape, got {tuple(p.shape)} and {tuple(t.shape)}")
    if p_np != t_np or (not p_np and p.device != t.device):
        raise ValueError(f"{who}: pred and target must be two numpy arrays or two tensors on one device")
    kernels = nnf.instance_supported(p, t)
    sides = []
    for m in (p, t):
        things_map, ign = _things_only(m, things, wide=not kernels)
        if kernels:
            roots = nnf.region_roots(things_map, conn, (ign,))
            ids, counts = nnf.region_ids(roots)
            table, moments = nnf.region_table(things_map, roots, ids, counts, capacity)
        else:
            roots = roots_torch(things_map, conn, (ign,))
            ids, counts = ids_torch(roots)
            table, moments = table_torch(things_map, roots, ids, capacity)
        sides.append((ids, counts, table, moments))
    (pi, pc, pt, pm), (gi, gc, gt, gm) = sides
    if kernels:
        cand, inter, void_count = nnf.instance_overlap(pi, gi, t, pt, gt, void, capacity)
        r = nnf.instance_tally(cand, inter, void_count, pt, gt, pc, gc, c)
    else:
        r, void_count = overlap_torch(pi, gi, t, pt, gt, pc, gc, void, capacity, c)
    return r, void_count, _regions_of(pt, pm, pc), _regions_of(gt, gm, gc), things, (p_np, p_single)


def match_regions(pred, target, num_classes: int, things=None, void=(255,), connectivity: int = 4, capacity: int = 1024) -> InstanceMatch:
    """The regions of the thing classes in `pred` and `target` -- class maps (B, H, W) or (H, W), tensors or numpy arrays -- and their
    one-to-one matching -> InstanceMatch(pred, target, match, inter, union, void, matched, overflow): both sides' Regions (utils.regions;
    `capacity` rows), match[g] the prediction id that ground-truth region g matches (equal class, 2 * inter > union with union =
    area[p] - void[p] + area[g] - inter) or -1, inter / union of the match, void[p] the pixels of prediction region p on a void target
    value, matched[p] whether prediction region p has a partner, overflow whether the image has more regions than rows on either side
    (it then matches nothing: raise `capacity`)."""
    r, void_count, pr, gr, _things, (is_np, single) = _run(pred, target, num_classes, things, void, connectivity, capacity, "match_regions")
    f = lambda x: _back(x, is_np, single)
    return InstanceMatch(Regions(*(f(x) for x in pr)), Regions(*(f(x) for x in gr)), f(r.match), f(r.inter), f(r.union), f(void_count),
                         f(r.matched), f(r.overflow))


def scores_from_tally(table, iou_sum, overflow, things) -> dict:
    """The data-set scores of (N, C, 5) counts, (N, C) IoU sums and (N,) overflow flags (numpy; host, float64): counts are summed over
    the images first (an overflowed image holds zeros), then per class RQ = tp / (tp + fp / 2 + fn / 2), SQ = iou_sum / tp, PQ = SQ *
    RQ, NaN where the denominator is 0 and for a class that is no thing; pq, sq, rq the means over the thing classes, NaN skipped (NaN
    when nothing is defined); count_errors the mean over the images that did not overflow of |n_pred - n_gt| per class, count_error its
    mean over the thing classes."""
    table, iou_sum, overflow = np.asarray(table, dtype=np.int64), np.asarray(iou_sum, dtype=np.float64), np.asarray(overflow) != 0
    c = table.shape[1]
    total = table.sum(axis=0)
    ious = np.zeros(c, dtype=np.float64)
    for row in iou_sum:                                     # image by image: a fixed order
        ious = ious + row
    tp, fp, fn = (total[:, k].astype(np.float64) for k in range(3))
    thing = np.zeros(c, dtype=bool)
    thing[list(things)] = True
    nan = np.full(c, np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = tp + fp / 2 + fn / 2
        rq = np.where(thing & (den > 0), tp / den, nan)
        sq = np.where(thing & (tp > 0), ious / tp, nan)
    pq = sq * rq
    seen = table[~overflow]
    errs = np.abs(seen[:, :, 3] - seen[:, :, 4]).mean(axis=0) if len(seen) else nan.copy()
    errs = np.where(thing, errs, nan)
    mean = lambda x: float(np.mean(x[~np.isnan(x)])) if (~np.isnan(x)).any() else float("nan")
    return dict(pq=mean(pq), sq=mean(sq), rq=mean(rq), pqs=pq, sqs=sq, rqs=rq, count_error=mean(errs), count_errors=errs,
                table=total.astype(np.int64), iou_sum=ious, images=int(table.shape[0]), overflowed=int(overflow.sum()))


def panoptic_stats(pred, target, num_classes: int, things=None, void=(255,), connectivity: int = 4, capacity: int = 1024) -> PanopticStats:
    """PanopticStats(table, iou_sum, overflow, pq, sq, rq, count_error) of class maps (B, H, W) or (H, W), tensors or numpy arrays:
    table (B, C, 5) int32 = (tp, fp, fn, n_pred, n_gt) per image and class, iou_sum (B, C) float64, overflow (B,) int32, and the float
    scores of the counts summed over THESE images (scores_from_tally; a data set goes through InstanceMeasurement)."""
    r, _void, _pr, _gr, things, (is_np, single) = _run(pred, target, num_classes, things, void, connectivity, capacity, "panoptic_stats")
    s = scores_from_tally(r.tally.cpu().numpy(), r.iou_sum.cpu().numpy(), r.overflow.cpu().numpy(), things)
    f = lambda x: _back(x, is_np, single)
    return PanopticStats(f(r.tally), f(r.iou_sum), f(r.overflow), s["pq"], s["sq"], s["rq"], s["count_error"])


def panoptic_quality(pred, target, num_classes: int, **settings) -> float:
    """panoptic_stats(...).pq"""
    return panoptic_stats(pred, target, num_classes, **settings).pq


class InstanceMeasurement:
    """Data-set-level panoptic quality: .update(pred_labels, target) once per batch (class maps (B, H, W), tensors or numpy arrays; only
    the (B, C, 5) counts, the (B, C) IoU sums and the (B,) flags leave the device), .result() the scores of the counts summed over all
    images seen:

        pq, sq, rq, count_error                      floats (NaN when nothing is defined)
        pqs, sqs, rqs, count_errors                  per-class float64 arrays (NaN for a class that is no thing)
        table (C, 5), iou_sum (C,)                   the summed counts (tp, fp, fn, n_pred, n_gt) and IoU sums
        images, overflowed                           how many images were seen, how many of them had more regions than `capacity`
    """

    def __init__(self, num_classes: int, things=None, void=(255,), connectivity: int = 4, capacity: int = 1024):
        self.num_classes, self.things, self.void, self.connectivity, self.capacity = nnf.instance_settings(
            num_classes, things, void, connectivity, capacity, "InstanceMeasurement")
        self.tables, self.iou_sums, self.overflows = [], [], []

    def update(self, pred_labels, target) -> None:
        r = _run(pred_labels, target, self.num_classes, self.things, self.void, self.connectivity, self.capacity, "InstanceMeasurement")[0]
        self.tables.append(r.tally.detach().cpu().numpy())
        self.iou_sums.append(r.iou_sum.detach().cpu().numpy())
        self.overflows.append(r.overflow.detach().cpu().numpy())

    def result(self) -> dict:
        c = self.num_classes
        table = np.concatenate(self.tables) if self.tables else np.zeros((0, c, 5), dtype=np.int32)
        iou_sum = np.concatenate(self.iou_sums) if self.iou_sums else np.zeros((0, c), dtype=np.float64)
        overflow = np.concatenate(self.overflows) if self.overflows else np.zeros((0,), dtype=np.int32)
        return scores_from_tally(table, iou_sum, overflow, self.things)
