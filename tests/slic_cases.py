"""The float64 numpy oracle of the SLIC / segment-mean kernels (include/vqseg.h states the algorithm; this restates it, sharing no code
with vq_seg_amd) and the cases the CPU and GPU tests run.  No parity with fast_slic or skimage is claimed or tested: neither exists
here.

The near-tie rule (a condition, not a measurement): where the oracle's best and second-best distance of a pixel differ by less than
NEAR_TIE = 1e-5 relative -- about 20 float32 roundings of a 5-term sum of squares -- the implementation may pick any candidate whose
oracle distance lies within that gap of the best; everywhere else its label must be the oracle's.  At most CAP = 0.5 % of a case's
pixels may be excused that way."""
import math

import numpy as np

NEAR_TIE = 1e-5
CAP = 0.005


# ---------------------------------------------------------------------------------------------------------------------- the oracle
def lab64(images, dtype=np.float64):
    """(B, 3, H, W) sRGB in [0, 1] -> CIELAB (B, 3, H, W); `dtype` float32 evaluates the same formulas in float32 numpy"""
    t = dtype
    v = np.asarray(images).astype(t)
    lin = np.where(v > t(0.04045), np.power((np.maximum(v, t(0)) + t(0.055)) / t(1.055), t(2.4)), v / t(12.92)).astype(t)
    r, g, b = lin[:, 0], lin[:, 1], lin[:, 2]
    x = (r * t(0.412453) + g * t(0.357580) + b * t(0.180423)) / t(0.95047)
    y = r * t(0.212671) + g * t(0.715160) + b * t(0.072169)
    z = (r * t(0.019334) + g * t(0.119193) + b * t(0.950227)) / t(1.08883)

    def f(u):
        return np.where(u > t(0.008856), np.cbrt(u), t(7.787) * u + t(16.0) / t(116.0)).astype(t)
    fx, fy, fz = f(x), f(y), f(z)
    return np.stack([t(116.0) * fy - t(16.0), t(500.0) * (fx - fy), t(200.0) * (fy - fz)], axis=1).astype(t)


def grid(h, w, k):
    """-> (gy, gx, S)"""
    s = math.sqrt(h * w / k)
    return max(1, int(round(h / s))), max(1, int(round(w / s))), s


def init_centers64(lab, gy, gx):
    """(B, gy * gx, 5): cluster (i, j) starts at pixel (floor((i + 1/2) H / gy), floor((j + 1/2) W / gx)) with its Lab value"""
    b, _, h, w = lab.shape
    out = np.zeros((b, gy * gx, 5), dtype=np.float64)
    for i in range(gy):
        for j in range(gx):
            y, x = ((2 * i + 1) * h) // (2 * gy), ((2 * j + 1) * w) // (2 * gx)
            out[:, i * gx + j, :3] = lab[:, :, y, x]
            out[:, i * gx + j, 3:] = (y, x)
    return out


def candidates64(lab, centers, gy, gx, compactness, s):
    """-> (index (9, H, W) int, distance (B, 9, H, W) float64, +inf where the cell does not exist), candidates in ascending index"""
    lab, centers = np.asarray(lab, dtype=np.float64), np.asarray(centers, dtype=np.float64)
    b, _, h, w = lab.shape
    hi, hj = (np.arange(h) * gy) // h, (np.arange(w) * gx) // w
    ys, xs = np.arange(h, dtype=np.float64)[:, None], np.arange(w, dtype=np.float64)[None, :]
    m2s = (compactness / s) ** 2
    index, dist = np.zeros((9, h, w), dtype=np.int64), np.full((b, 9, h, w), np.inf)
    at = 0
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ci, cj = hi + di, hj + dj
            ok = ((ci >= 0) & (ci < gy))[:, None] & ((cj >= 0) & (cj < gx))[None, :]
            idx = np.clip(ci, 0, gy - 1)[:, None] * gx + np.clip(cj, 0, gx - 1)[None, :]
            c = centers[:, idx]                                                      # (B, H, W, 5)
            d = ((lab[:, 0] - c[..., 0]) ** 2 + (lab[:, 1] - c[..., 1]) ** 2 + (lab[:, 2] - c[..., 2]) ** 2
                 + m2s * ((ys - c[..., 3]) ** 2 + (xs - c[..., 4]) ** 2))
            index[at], dist[:, at] = idx, np.where(ok, d, np.inf)
            at += 1
    return index, dist


def assign64(lab, centers, gy, gx, compactness, s):
    """-> (labels (B, H, W) int64, best distance, second-best distance (+inf where there is one candidate)); ties to the lowest index"""
    index, dist = candidates64(lab, centers, gy, gx, compactness, s)
    first = np.argmin(dist, axis=1)                                                  # the first minimum: the lowest index
    labels = np.take_along_axis(np.broadcast_to(index, dist.shape), first[:, None], axis=1)[:, 0]
    two = np.sort(dist, axis=1)[:, :2]
    return labels, two[:, 0], two[:, 1]


def update64(lab, labels, centers):
    """the mean of (L, a, b, y, x) over each cluster's pixels; an empty cluster keeps its centre.  -> (centers, counts (B, K))"""
    lab = np.asarray(lab, dtype=np.float64)
    b, _, h, w = lab.shape
    out = np.array(centers, dtype=np.float64)
    k = out.shape[1]
    ys, xs = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w)), np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    counts = np.zeros((b, k), dtype=np.int64)
    for n in range(b):
        vals = np.stack([lab[n, 0], lab[n, 1], lab[n, 2], ys, xs], axis=-1).reshape(-1, 5)
        at = np.asarray(labels[n]).reshape(-1)
        counts[n] = np.bincount(at, minlength=k)
        for v in range(5):
            sums = np.bincount(at, weights=vals[:, v], minlength=k)
            out[n, counts[n] > 0, v] = sums[counts[n] > 0] / counts[n][counts[n] > 0]
    return out, counts


def segment_mean64(x, labels, k):
    """y[b, :, p] = the mean of x[b, :, q] over the q with labels[b, q] == labels[b, p]; labels outside [0, k) pass through.
    -> (y float64, per-pixel count of the pixel's segment (1 for passed-through pixels))"""
    x = np.asarray(x, dtype=np.float64)
    labels = np.asarray(labels).astype(np.int64)
    b, c, h, w = x.shape
    y, cnt = x.copy(), np.ones((b, h, w), dtype=np.int64)
    for n in range(b):
        at = labels[n].reshape(-1)
        ok = (at >= 0) & (at < k)
        counts = np.bincount(at[ok], minlength=k)
        cnt[n].reshape(-1)[ok] = counts[at[ok]]
        for ch in range(c):
            sums = np.bincount(at[ok], weights=x[n, ch].reshape(-1)[ok], minlength=k)
            y[n, ch].reshape(-1)[ok] = sums[at[ok]] / counts[at[ok]]
    return y, cnt


def update_bound(lab, labels, k):
    """n_k * 2^-23 * max|value| per cluster and component (B, K, 5), the values being (L, a, b, y, x) of the cluster's pixels: any-order
    float32 summation followed by one division (see mean_bound); 0 for an empty cluster, which must keep its centre bit for bit"""
    lab = np.asarray(lab, dtype=np.float64)
    b, _, h, w = lab.shape
    ys, xs = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w)), np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    out = np.zeros((b, k, 5))
    for n in range(b):
        at = np.asarray(labels[n]).reshape(-1).astype(np.int64)
        counts = np.bincount(at, minlength=k)
        for v, plane in enumerate((lab[n, 0], lab[n, 1], lab[n, 2], ys, xs)):
            top = np.zeros(k)
            np.maximum.at(top, at, np.abs(plane).reshape(-1))
            out[n, :, v] = counts * 2.0 ** -23 * top
    return out


def slic64(images, k, compactness=10.0, iters=10):
    """the whole loop in float64 -> (labels, centers, (gy, gx))"""
    b, _, h, w = images.shape
    gy, gx, s = grid(h, w, k)
    lab = lab64(images)
    centers = init_centers64(lab, gy, gx)
    for _ in range(iters):
        centers = update64(lab, assign64(lab, centers, gy, gx, compactness, s)[0], centers)[0]
    return assign64(lab, centers, gy, gx, compactness, s)[0], centers, (gy, gx)


def excused(got, lab, centers, gy, gx, compactness, s):
    """the near-tie rule -> (excused count, violations count) of labels `got` (B, H, W) against assign64 on (lab, centers).  A pixel
    whose label differs from the oracle's is excused if the oracle's two best distances lie within NEAR_TIE (relative) of each other
    and the distance of the chosen cluster lies within that gap of the best; a label that is no candidate is a violation."""
    index, dist = candidates64(lab, centers, gy, gx, compactness, s)
    want, best, second = assign64(lab, centers, gy, gx, compactness, s)
    got = np.asarray(got).astype(np.int64)
    differs = got != want
    is_cand = (np.broadcast_to(index, dist.shape) == got[:, None]) & np.isfinite(dist)
    chosen = np.where(is_cand, dist, np.inf).min(axis=1)                             # +inf: not a candidate at all
    gap = NEAR_TIE * np.maximum(best, np.finfo(np.float64).tiny)
    near = (second - best < gap) & (chosen - best < gap)
    return int((differs & near).sum()), int((differs & ~near).sum())


# ------------------------------------------------------------------------------------------------------------------------ the cases
def noise(seed, b, h, w):
    """uniform random rounded to k / 255"""
    return (np.random.default_rng(seed).integers(0, 256, size=(b, 3, h, w)) / 255.0).astype(np.float32)


def smooth(seed, b, h, w):
    """three sinusoid / ramp channels plus 10 % noise"""
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([0.5 + 0.5 * np.sin(ys / 5.0 + xs / 9.0), xs / max(w - 1, 1), 0.5 + 0.5 * np.cos(ys / 7.0 - xs / 4.0)])
    img = 0.9 * base[None] + 0.1 * np.random.default_rng(seed).random((b, 3, h, w))
    return np.clip(img, 0.0, 1.0).astype(np.float32)


def _case1():
    return np.concatenate([noise(101, 1, 37, 53), smooth(102, 1, 37, 53)])


def _case5():
    img = np.zeros((1, 3, 40, 40), dtype=np.float32)
    img[..., 17:] = 1.0
    return img


# name -> (images float32 (B, 3, H, W), K, compactness, the grid the issue states or None)
CASES = {
    "1-odd-sides": (_case1(), 24, 10.0, (4, 6)),
    "2-one-row": (noise(201, 1, 16, 40), 3, 10.0, (1, 3)),
    "3-one-cluster": (noise(301, 1, 24, 24), 1, 10.0, (1, 1)),
    "4a-keff-smooth": (smooth(401, 1, 64, 48), 60, 1.0, (9, 7)),
    "4b-keff-noise": (noise(402, 1, 64, 48), 60, 40.0, (9, 7)),
    "5-edge": (_case5(), 16, 10.0, None),
    "6-constant": (np.full((1, 3, 64, 64), 100.0 / 255.0, dtype=np.float32), 16, 10.0, None),
}


def arbitrary_labels(seed=7, b=2, h=37, w=53, k=40):
    """an adversarial label map: a random permutation of labels with one segment of a single pixel (label 0), one unused index (1)
    and one pixel of label k, which must pass through unchanged.  -> (labels int32 (B, H, W), k)"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(2, k, size=(b, h, w))
    for n in range(b):
        lab[n] = rng.permutation(lab[n].reshape(-1)).reshape(h, w)
        lab[n, rng.integers(h), rng.integers(w)] = 0
        y, x = rng.integers(h), rng.integers(w)
        if lab[n, y, x] == 0:
            x = (x + 1) % w
        lab[n, y, x] = k
    return lab.astype(np.int32), k


def mean_bound(x, labels, k):
    """n_k * 2^-23 * max|x| per segment and channel, at every pixel (B, C, H, W): any-order float32 summation of the segment's n_k values
    ((n_k - 1) 2^-24 sum|x| <= (n_k - 1) 2^-24 n_k max|x|) followed by one division by n_k and its rounding; 0 for passed-through pixels"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    labels = np.asarray(labels).astype(np.int64)
    b, c, h, w = x.shape
    out = np.zeros_like(x)
    for n in range(b):
        at = labels[n].reshape(-1)
        ok = (at >= 0) & (at < k)
        counts = np.bincount(at[ok], minlength=k)
        for ch in range(c):
            top = np.zeros(k)
            np.maximum.at(top, at[ok], x[n, ch].reshape(-1)[ok])
            out[n, ch].reshape(-1)[ok] = (counts * 2.0 ** -23 * top)[at[ok]]
    return out
