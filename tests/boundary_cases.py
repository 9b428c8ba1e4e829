"""The definition of include/vqseg.h's boundary metrics, restated in plain numpy, and the case table of the boundary suites
(tests/test_boundary_cpu.py, tests/test_boundary_kernel_gpu.py, tests/test_boundary_eval_gpu.py).  Nothing of vq_seg_amd is imported
here; the patterns are those of tests/region_cases.py.

    boundaries(labels, num_classes, ignore)                 (B, C, H, W) uint8 of 0 / 1
    edt_sq(seeds)                                           (..., H, W) int32; EDT_NONE on a plane without a seed
    counts(pred, target, num_classes, tol_sq, width_sq, ignore)   (B, C, 8) int32
    scores(table)                                           dict of (B, C) float64 arrays, NaN where undefined
    nanmean_classes(x)                                      the data-set mean of a (N, C) score: (mean, per class)

edt_sq is the brute-force minimum over all seeds, taken row by row: min over q = min over the rows j of (min over the seeds q of row j
of (px - qx)^2) + (py - j)^2 -- the same minimum, every seed looked at, in int64.  All of it is integer arithmetic up to the scores:
every comparison against it is exact."""
import functools

import numpy as np

from tests import region_cases as rc

EDT_NONE = 2 ** 31 - 1
NUM_CLASSES = 3
IGNORE = (255,)
PATTERN_NAMES = ["random41", "random50", "rings", "diagonal", "comb", "spiral", "checkerboard", "constant", "ignored"]
SHAPES = [(1, 1), (1, 70), (70, 1), (17, 65), (33, 130), (67, 259), (300, 5), (5, 300)]
SETTINGS = [(0, 1), (1, 1), (2, 3), (3.5, 3.5)]                 # (tolerance, width); floor(3.5^2) = 12 catches a rounded-up threshold


def squared(x):
    return int(np.floor(float(x) ** 2))


def boundaries(labels, num_classes, ignore=()):
    labels = np.asarray(labels)
    b, h, w = labels.shape
    v = labels.astype(np.int64)
    out = np.zeros((b, num_classes, h, w), dtype=np.uint8)
    for c in range(num_classes):
        edge = np.zeros((b, h, w), dtype=bool)
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            q = np.full((b, h, w), c, dtype=np.int64)            # outside the image: the class itself, which makes no boundary
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            q[:, yd, xd] = v[:, ys, xs]
            other = q != c
            for i in ignore:
                other &= q != int(i)
            edge |= other
        out[:, c] = (v == c) & edge
    return out


def edt_sq_plane(s):
    """one seed plane (H, W) -> (H, W) int32"""
    h, w = s.shape
    big = np.int64(1) << 40
    x = np.arange(w, dtype=np.int64)
    gx = np.full((h, w), big, dtype=np.int64)                    # per row: the smallest (px - qx)^2 over the row's seeds
    for j in range(h):
        at = np.nonzero(s[j])[0].astype(np.int64)
        if len(at):
            gx[j] = ((x[:, None] - at[None, :]) ** 2).min(axis=1)
    if (gx >= big).all():
        return np.full((h, w), EDT_NONE, dtype=np.int32)
    y = np.arange(h, dtype=np.int64)
    out = np.empty((h, w), dtype=np.int64)
    for y0 in range(0, h, 32):                                   # (a block of rows at a time: memory, nothing else)
        dy2 = (y[y0:y0 + 32, None] - y[None, :]) ** 2            # (rows, j)
        out[y0:y0 + 32] = (gx[None, :, :] + dy2[:, :, None]).min(axis=1)
    return out.astype(np.int32)


def edt_sq(seeds):
    seeds = np.asarray(seeds)
    h, w = seeds.shape[-2:]
    flat = seeds.reshape(-1, h, w)
    return np.stack([edt_sq_plane(p != 0) for p in flat]).reshape(seeds.shape).astype(np.int32)


def counts(pred, target, num_classes, tol_sq, width_sq, ignore=(), parts=None):
    """parts: (bp, bg, dp, dg) where they are at hand already (they do not depend on the thresholds)"""
    pred, target = np.asarray(pred).astype(np.int64), np.asarray(target).astype(np.int64)
    b = pred.shape[0]
    if parts is None:
        bp, bg = boundaries(pred, num_classes, ignore), boundaries(target, num_classes, ignore)
        parts = (bp, bg, edt_sq(bp), edt_sq(bg))
    bp, bg, dp, dg = parts
    valid = np.ones(target.shape, dtype=bool)
    for i in ignore:
        valid &= target != int(i)
    table = np.zeros((b, num_classes, 8), dtype=np.int32)
    for k in range(b):
        for c in range(num_classes):
            p_edge, g_edge = valid[k] & (bp[k, c] != 0), valid[k] & (bg[k, c] != 0)
            pd = valid[k] & (pred[k] == c) & (dp[k, c] <= width_sq)
            gd = valid[k] & (target[k] == c) & (dg[k, c] <= width_sq)
            row = table[k, c]
            row[0], row[1] = p_edge.sum(), (p_edge & (dg[k, c] <= tol_sq)).sum()
            row[2], row[3] = g_edge.sum(), (g_edge & (dp[k, c] <= tol_sq)).sum()
            row[4], row[5] = (pd & gd).sum(), (pd | gd).sum()
            row[6] = -1 if row[0] == 0 or not bg[k, c].any() else dg[k, c][p_edge].max()
            row[7] = -1 if row[2] == 0 or not bp[k, c].any() else dp[k, c][g_edge].max()
    return table


def scores(table):
    """(B, C, 8) -> dict(precision, recall, f1, iou, hausdorff), each (B, C) float64 with NaN where undefined"""
    t = np.asarray(table).astype(np.float64)
    shape = t.shape[:-1]
    out = {k: np.full(shape, np.nan) for k in ("precision", "recall", "f1", "iou", "hausdorff")}
    for idx in np.ndindex(*shape):
        n_pred, hit_pred, n_gt, hit_gt, inter, union, hd_p, hd_g = t[idx]
        p = hit_pred / n_pred if n_pred > 0 else np.nan
        r = hit_gt / n_gt if n_gt > 0 else np.nan
        out["precision"][idx], out["recall"][idx] = p, r
        if n_pred == 0 and n_gt == 0:
            f = np.nan
        elif n_pred == 0 or n_gt == 0 or p + r == 0:
            f = 0.0
        else:
            f = 2 * p * r / (p + r)
        out["f1"][idx] = f
        out["iou"][idx] = inter / union if union > 0 else np.nan
        out["hausdorff"][idx] = np.sqrt(max(hd_p, hd_g)) if hd_p >= 0 and hd_g >= 0 else np.nan
    return out


def nanmean_classes(x):
    """(N, C) scores over all images -> (the mean over the classes that are defined for some image, the per-class means): a class
    that is NaN for every image is NaN in the list and left out of the mean; the mean of nothing is NaN"""
    x = np.asarray(x, dtype=np.float64)
    per = np.array([np.nan if np.isnan(x[:, c]).all() else np.nanmean(x[:, c]) for c in range(x.shape[1])])
    return (np.nan if np.isnan(per).all() else float(np.nanmean(per))), per


# ------------------------------------------------------------------------------------------------------------------------------
# cases: name -> (pred, target), both (B, H, W) uint8 with values in {0, 1, 2} and 255
# ------------------------------------------------------------------------------------------------------------------------------
def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pair(name):
    if name == "batch":
        target = rc.batch_case()
        pred = np.roll(target, (1, 2), axis=(1, 2))
    else:
        pattern, shape = name.rsplit("-", 1)
        h, w = (int(s) for s in shape.split("x"))
        if pattern == "random41v50":
            pred, target = rc.PATTERNS["random41"](h, w)[None], rc.PATTERNS["random50"](h, w)[None]
        else:
            target = rc.PATTERNS[pattern](h, w)[None]
            pred = np.roll(target, (1, 2), axis=(1, 2))
    return _readonly(np.ascontiguousarray(pred, dtype=np.uint8), np.ascontiguousarray(target, dtype=np.uint8))


CASES = [f"{p}-{h}x{w}" for p in PATTERN_NAMES + ["random41v50"] for h, w in SHAPES] + ["batch"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """everything the definition gives for a case that does not depend on the thresholds, computed once and shared (read-only)"""
    pred, target = pair(name)
    bp, bg = boundaries(pred, NUM_CLASSES, IGNORE), boundaries(target, NUM_CLASSES, IGNORE)
    out = dict(pred=pred, target=target, bp=bp, bg=bg, dp=edt_sq(bp), dg=edt_sq(bg))
    _readonly(*(v for k, v in out.items() if k not in ("pred", "target")))
    return out


@functools.lru_cache(maxsize=None)
def reference_counts(name, tolerance, width):
    ref = reference(name)
    parts = (ref["bp"], ref["bg"], ref["dp"], ref["dg"])
    return _readonly(counts(ref["pred"], ref["target"], NUM_CLASSES, squared(tolerance), squared(width), IGNORE, parts))[0]


def lone_seed(h, w, y, x):
    s = np.zeros((h, w), dtype=np.uint8)
    s[y, x] = 1
    return s


def first_and_last_row(h, w):
    s = np.zeros((h, w), dtype=np.uint8)
    s[0, ::2] = 1
    s[-1, 1::3] = 1
    return s


SEED_PLANES = {
    "lone-first": lambda: lone_seed(257, 259, 0, 0),             # the far corner reads 256^2 + 258^2 = 132100
    "lone-last": lambda: lone_seed(257, 259, 256, 258),
    "first-and-last-row": lambda: first_and_last_row(300, 5),
}


@functools.lru_cache(maxsize=None)
def seed_plane(name):
    s = SEED_PLANES[name]()
    return _readonly(s, edt_sq(s))
