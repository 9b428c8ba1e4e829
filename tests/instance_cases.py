"""The definition of include/vqseg.h's panoptic quality, restated in plain numpy, and the case table of the instance suites
(tests/test_instances_cpu.py, tests/test_instances_kernel_gpu.py, tests/test_instances_eval_gpu.py).  Nothing of vq_seg_amd is
imported here.  The regions are those of tests/region_cases.py's union-find; the matching is brute force over ALL pairs (g, p) of
equal value with 2 * inter > union -- no majority rule -- and asserts that a region has at most one partner.

    things_map(v, things)                                  int64 map, -1 where the value is no thing class
    side(values, things, connectivity, capacity)           (ids, counts, table) of the thing regions of one map
    match_from(pred_id, gt_id, target, ptab, gtab, pcount, gcount, void, capacity, num_classes)
                                                           dict(match, inter, union, void, matched, tally, iou_sum, overflow)
    scores(tally, iou_sum, overflow, things)               dict(pq, sq, rq, pqs, sqs, rqs, count_error, count_errors)

All tables are integers: every comparison against them is exact.  iou_sum is a float64 sum in rising ground-truth id."""
import functools

import numpy as np

from tests import region_cases as rc

NUM_CLASSES = 3
VOID = (255,)


def things_map(v, things):
    v = np.asarray(v).astype(np.int64)
    return np.where(np.isin(v, np.asarray(list(things), dtype=np.int64)), v, -1)


def side(v, things, connectivity, capacity):
    m = things_map(v, things)
    roots = rc.roots(m, connectivity, (-1,))
    ids, counts = rc.ids(roots)
    table, _moments = rc.table(m, roots, ids, capacity)
    return ids, counts, table


def match_from(pred_id, gt_id, target, ptab, gtab, pcount, gcount, void, capacity, num_classes):
    b = pred_id.shape[0]
    out = dict(match=np.full((b, capacity), -1, dtype=np.int32), inter=np.zeros((b, capacity), dtype=np.int32),
               union=np.zeros((b, capacity), dtype=np.int32), void=np.zeros((b, capacity), dtype=np.int32),
               matched=np.zeros((b, capacity), dtype=np.int32), tally=np.zeros((b, num_classes, 5), dtype=np.int32),
               iou_sum=np.zeros((b, num_classes), dtype=np.float64), overflow=np.zeros(b, dtype=np.int32))
    for k in range(b):
        p, g, t = pred_id[k].reshape(-1).astype(np.int64), gt_id[k].reshape(-1).astype(np.int64), target[k].reshape(-1).astype(np.int64)
        pok, gok = (p >= 0) & (p < capacity), (g >= 0) & (g < capacity)
        at = pok & ~gok & np.isin(t, np.asarray(list(void), dtype=np.int64))
        out["void"][k] = np.bincount(p[at], minlength=capacity)
        if pcount[k] > capacity or gcount[k] > capacity:
            out["overflow"][k] = 1
            continue
        n_p, n_g = max(int(pcount[k]), 0), max(int(gcount[k]), 0)
        both = pok & gok
        inter = np.zeros((capacity, capacity), dtype=np.int64)
        np.add.at(inter, (g[both], p[both]), 1)
        inter = inter[:n_g, :n_p]
        pv, pa, vd = (x.astype(np.int64) for x in (ptab[k, :n_p, 0], ptab[k, :n_p, 1], out["void"][k, :n_p]))
        gv, ga = gtab[k, :n_g, 0].astype(np.int64), gtab[k, :n_g, 1].astype(np.int64)
        union = pa[None, :] - vd[None, :] + ga[:, None] - inter
        ok = (pv[None, :] == gv[:, None]) & (2 * inter > union)                 # every pair, strict
        assert (ok.sum(axis=0) <= 1).all() and (ok.sum(axis=1) <= 1).all(), "a region with two partners"
        gs, ps = np.nonzero(ok)
        out["match"][k, gs], out["inter"][k, gs], out["union"][k, gs] = ps, inter[gs, ps], union[gs, ps]
        out["matched"][k, ps] = 1
        for r in range(n_g):                                                    # rising ground-truth id
            c = int(gv[r])
            if 0 <= c < num_classes:
                out["tally"][k, c, 4] += 1
                if out["match"][k, r] >= 0:
                    out["tally"][k, c, 0] += 1
                    out["iou_sum"][k, c] += np.float64(out["inter"][k, r]) / np.float64(out["union"][k, r])
                else:
                    out["tally"][k, c, 2] += 1
        for r in range(n_p):
            c = int(pv[r])
            if 0 <= c < num_classes:
                out["tally"][k, c, 3] += 1
                if not out["matched"][k, r] and 2 * vd[r] <= pa[r]:
                    out["tally"][k, c, 1] += 1
    return out


def scores(tally, iou_sum, overflow, things):
    c = tally.shape[1]
    total = tally.astype(np.int64).sum(axis=0)
    ious = np.zeros(c)
    for row in iou_sum:
        ious = ious + row
    out = {key: np.full(c, np.nan) for key in ("pqs", "sqs", "rqs", "count_errors")}
    seen = tally[np.asarray(overflow) == 0].astype(np.int64)
    for k in things:
        tp, fp, fn = (float(x) for x in total[k, :3])
        if tp + fp / 2 + fn / 2 > 0:
            out["rqs"][k] = tp / (tp + fp / 2 + fn / 2)
        if tp > 0:
            out["sqs"][k] = ious[k] / tp
        out["pqs"][k] = out["sqs"][k] * out["rqs"][k]
        if len(seen):
            out["count_errors"][k] = np.abs(seen[:, k, 3] - seen[:, k, 4]).mean()
    for key in ("pq", "sq", "rq", "count_error"):
        x = out[key + "s"]
        out[key] = float(np.mean(x[~np.isnan(x)])) if (~np.isnan(x)).any() else float("nan")
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# patterns: (H, W) uint8 maps with values in {0, 1, 2}, 255 and (one case) 7
# ------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([0x1A57] + [int(k) for k in key])


def blobs(h, w, seed):
    """rectangles of class 1 and 2 on 0, up to a third of the image each: some overlap into odd shapes, the large ones exceed 256 pixels"""
    g = _rng(h, w, seed)
    v = np.zeros((h, w), dtype=np.uint8)
    for k in range(max(1, h * w // 300)):
        bh, bw = int(g.integers(1, max(2, h // 3 + 1))), int(g.integers(1, max(2, w // 3 + 1)))
        y, x = int(g.integers(0, h - bh + 1)), int(g.integers(0, w - bw + 1))
        v[y:y + bh, x:x + bw] = 1 + k % 2
    return v


def shift(v, dy, dx, fill=0):
    h, w = v.shape
    out = np.full_like(v, fill)
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[yd, xd] = v[ys, xs]
    return out


def speckle(v, seed, rate=0.01):
    g = _rng(v.shape[0], v.shape[1], seed, 77)
    out = v.copy()
    at = g.random(v.shape) < rate
    out[at] = g.integers(0, 3, size=v.shape)[at].astype(np.uint8)
    return out


def with_void(v, seed, rate=0.02):
    g = _rng(v.shape[0], v.shape[1], seed, 255)
    out = v.copy()
    out[g.random(v.shape) < rate] = 255
    return out


def _canvas(h=33, w=65):
    return np.zeros((h, w), dtype=np.uint8), np.zeros((h, w), dtype=np.uint8)


def exact_half():
    """class 1: areas 300 and 300, inter 200, union 400: 2 * inter == union, no match.  Class 2: one pixel more in both: 402 > 401."""
    p, t = _canvas()
    t[0:10, 0:30], p[0:10, 10:40] = 1, 1
    t[15:25, 0:30], p[15:25, 10:40] = 2, 2
    t[25, 15], p[25, 15] = 2, 2
    return p, t


def split2():
    """a ground-truth region of 300 in two prediction pieces of 200 (a match: 400 > 300) and 90 (invented)"""
    p, t = _canvas()
    t[2:12, 3:33] = 1
    p[2:12, 3:23], p[2:12, 24:33] = 1, 1
    return p, t


def split3():
    """three pieces of 100 each of a region of 320: no majority.  The bits of ids 0, 1, 2 (+ 1) assemble id 2: a garbage candidate"""
    p, t = _canvas()
    t[2:12, 3:35] = 1
    p[2:12, 3:13], p[2:12, 14:24], p[2:12, 25:35] = 1, 1, 1
    t[20:25, 40:50], p[20:25, 40:50] = 2, 2                                     # and an ordinary match beside it
    return p, t


def merged():
    """one prediction region of 260 over ground-truth regions of 200 (a match: 400 > 260) and 50 (missed)"""
    p, t = _canvas()
    t[5:15, 0:20], t[5:15, 21:26] = 1, 1
    p[5:15, 0:26] = 1
    return p, t


def wrong_class():
    """the majority region has another class: no match, one missed of class 1, one invented of class 2"""
    p, t = _canvas()
    t[5:15, 5:25], p[5:15, 5:25] = 1, 2
    t[20:30, 30:60], p[20:30, 31:60] = 2, 2
    return p, t


def mostly_void():
    """prediction regions on void: 60 of 100 pixels (dropped, no fp), exactly 50 of 100 (kept: an fp), and 30 of 100"""
    p, t = _canvas()
    for k, n_void in enumerate((6, 5, 3)):
        x0 = 20 * k
        p[3:13, x0:x0 + 10] = 1
        t[3:13, x0:x0 + n_void] = 255
    t[20:30, 5:25], p[20:30, 5:25] = 2, 2
    return p, t


def void_trim():
    """class 1: ground truth 100, prediction 300 of which 200 on void (255 and 7): union 100, a match.  Class 2: the same without void: none"""
    p, t = _canvas()
    t[0:10, 0:10], p[0:10, 0:30] = 1, 1
    t[0:10, 10:20], t[0:10, 20:30] = 255, 7
    t[15:25, 0:10], p[15:25, 0:30] = 2, 2
    return p, t


def lattice(h, w):
    """isolated pixels at even rows and columns, classes 1 and 2 by turns"""
    v = np.zeros((h, w), dtype=np.uint8)
    ys, xs = np.meshgrid(np.arange(0, h, 2), np.arange(0, w, 2), indexing="ij")
    v[ys, xs] = 1 + (ys // 2 + xs // 2) % 2
    return v


def lattice_pair(h, w, swap=False):
    """ground truth: the lattice.  Prediction: the lattice with every seventh pixel missing and every fifth of the other class.
    `swap`: the other way round"""
    t = lattice(h, w)
    p = t.copy()
    ys, xs = np.nonzero(t)
    k = np.arange(len(ys))
    p[ys[k % 7 == 3], xs[k % 7 == 3]] = 0
    sel = (k % 5 == 1) & (k % 7 != 3)
    p[ys[sel], xs[sel]] = 3 - t[ys[sel], xs[sel]]
    return (t, p) if swap else (p, t)


def row_runs(n):
    t = np.zeros(n, dtype=np.uint8)
    t[0:30], t[35:60] = 1, 2
    p = np.zeros(n, dtype=np.uint8)
    p[3:33], p[33:58] = 1, 2
    return p, t


def _pair(p, t):
    return np.ascontiguousarray(p, dtype=np.uint8)[None], np.ascontiguousarray(t, dtype=np.uint8)[None]


def _shifted(h, w, seed, dy, dx, noise=True):
    t = blobs(h, w, seed)
    p = shift(t, dy, dx)
    return _pair(speckle(p, seed) if noise else p, with_void(t, seed) if noise else t)


def _batch(middle=None):
    h, w = 40, 72
    ps, ts = [], []
    for k, (dy, dx) in enumerate(((0, 1), (2, -3), (1, 1))):
        p, t = _shifted(h, w, 40 + k, dy, dx)
        ps.append(p[0]), ts.append(t[0])
    if middle is not None:
        ps[1], ts[1] = middle
    return np.stack(ps), np.stack(ts)


def _nothing(h, w):
    t = np.zeros((h, w), dtype=np.uint8)
    t[::3, ::5] = 255
    return _pair(np.zeros((h, w), dtype=np.uint8), t)


# name -> (maker of (pred, target) uint8 (B, H, W), things or None for the default, void, capacity, overflows).  The capacities of the
# cases that must not overflow lie at or above the largest region count of either side for both connectivities (tests/test_instances_cpu.py
# verifies it); "lattice-exact" has count == capacity on the ground-truth side, the overflow cases count == capacity + 1.
CASES = {
    "one-1x1": (lambda: _pair(np.ones((1, 1)), np.ones((1, 1))), None, VOID, 4, False),
    "runs-1x70": (lambda: _pair(*(x[None, :] for x in row_runs(70))), None, VOID, 8, False),
    "runs-70x1": (lambda: _pair(*(x[:, None] for x in row_runs(70))), None, VOID, 8, False),
    "identical-33x65": (lambda: _pair(rc.random3(33, 65, 0.59, 3), rc.random3(33, 65, 0.59, 3)), None, VOID, 512, False),
    "identical-blobs-130x130": (lambda: _pair(blobs(130, 130, 1), blobs(130, 130, 1)), None, VOID, 64, False),
    "shift1-33x65": (lambda: _shifted(33, 65, 2, 0, 1), None, VOID, 64, False),
    "shift3-67x131": (lambda: _shifted(67, 131, 3, 2, 3), None, VOID, 256, False),
    "shift-130x130": (lambda: _shifted(130, 130, 4, 1, -2), None, VOID, 512, False),
    "random-130x130": (lambda: _pair(rc.random3(130, 130, 0.59, 1), rc.random3(130, 130, 0.59, 2)), None, VOID, 4096, False),
    "exact-half": (lambda: _pair(*exact_half()), None, VOID, 16, False),
    "split2": (lambda: _pair(*split2()), None, VOID, 16, False),
    "split3": (lambda: _pair(*split3()), None, VOID, 16, False),
    "merged": (lambda: _pair(*merged()), None, VOID, 16, False),
    "wrong-class": (lambda: _pair(*wrong_class()), None, VOID, 16, False),
    "mostly-void": (lambda: _pair(*mostly_void()), None, VOID, 16, False),
    "void-trim": (lambda: _pair(*void_trim()), None, (255, 7), 16, False),
    "checkerboard-33x65": (lambda: _pair(rc.checkerboard(33, 65), shift(rc.checkerboard(33, 65), 0, 2)), None, VOID, 1100, False),
    "lattice-exact": (lambda: _pair(*lattice_pair(33, 65)), None, VOID, 561, False),
    "lattice-gt-over": (lambda: _pair(*lattice_pair(33, 65)), None, VOID, 560, True),
    "lattice-pred-over": (lambda: _pair(*lattice_pair(33, 65, swap=True)), None, VOID, 560, True),
    "nothing-33x65": (lambda: _nothing(33, 65), None, VOID, 8, False),
    "things2-67x131": (lambda: _shifted(67, 131, 3, 2, 3), (2,), VOID, 256, False),
    "things012-33x65": (lambda: _shifted(33, 65, 5, 1, 0), (0, 1, 2), VOID, 128, False),
    "batch": (lambda: _batch(), None, VOID, 256, False),
    "batch-lattice": (lambda: _batch(lattice_pair(40, 72)), None, VOID, 720, False),
    "batch-lattice-over": (lambda: _batch(lattice_pair(40, 72)), None, VOID, 719, True),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (pred, target) uint8 (B, H, W), read-only"""
    p, t = CASES[name][0]()
    assert p.dtype == np.uint8 and t.dtype == np.uint8 and p.shape == t.shape and p.ndim == 3
    p.setflags(write=False), t.setflags(write=False)
    return p, t


def settings(name):
    """(things, void, capacity, overflows) of a case, things resolved"""
    _make, things, void, capacity, overflows = CASES[name]
    return tuple(range(1, NUM_CLASSES)) if things is None else things, void, capacity, overflows


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """everything the definition gives for a case, computed once and shared (read-only arrays)"""
    p, t = case(name)
    things, void, capacity, _over = settings(name)
    pid, pcount, ptab = side(p, things, connectivity, capacity)
    gid, gcount, gtab = side(t, things, connectivity, capacity)
    out = match_from(pid, gid, t, ptab, gtab, pcount, gcount, void, capacity, NUM_CLASSES)
    out.update(pred=p, target=t, pred_id=pid, gt_id=gid, pred_count=pcount, gt_count=gcount, pred_table=ptab, gt_table=gtab)
    for x in out.values():
        x.setflags(write=False)
    out["scores"] = scores(out["tally"], out["iou_sum"], out["overflow"], things)
    return out
