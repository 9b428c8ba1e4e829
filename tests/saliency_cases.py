"""The float64 numpy restatement of RBD saliency over a SLIC label map (include/vqseg.h states the definition; this restates it, sharing no
code with vq_seg_amd), stage by stage so that a stage can be judged on given inputs, and the cases the CPU and GPU tests run: a
synthetic Lab image and a jittered-grid label map, in which every pixel's label is a cluster of the 3 x 3 cells around its home cell,
as in a map that slic made.  No parity with the reference's saliency numbers is claimed or tested (its superpixels are skimage's)."""
import functools
import math

import numpy as np

SIGMA_CLR, SIGMA_BNDCON, SIGMA_SPA, MU = 10.0, 1.0, 0.25, 0.1


# ---------------------------------------------------------------------------------------------------------------- the restatement
def valid_labels(labels, gy, gx):
    """int64 labels with -1 where the label names no cluster of the 3 x 3 cells around the pixel's home cell (such a pixel belongs to
    no cluster, is nobody's neighbour and is painted 0)"""
    lv = np.asarray(labels).astype(np.int64)
    _, h, w = lv.shape
    hi, hj = (np.arange(h) * gy) // h, (np.arange(w) * gx) // w
    inside = (lv >= 0) & (lv < gy * gx)
    ci, cj = np.where(inside, lv, 0) // gx, np.where(inside, lv, 0) % gx
    ok = inside & (np.abs(ci - hi[None, :, None]) <= 1) & (np.abs(cj - hj[None, None, :]) <= 1)
    return np.where(ok, lv, -1)


def region64(lab, labels, gy, gx):
    """-> (stats (B, K, 8) = (L, a, b, y, x, n, bnd, 0) float64, adj (B, K, K) uint8)"""
    lab = np.asarray(lab, dtype=np.float64)
    b, _, h, w = lab.shape
    k = gy * gx
    lv = valid_labels(labels, gy, gx)
    stats, adj = np.zeros((b, k, 8)), np.zeros((b, k, k), dtype=np.uint8)
    ys, xs = np.mgrid[:h, :w]
    for n in range(b):
        for c in range(k):
            at = lv[n] == c
            cnt = int(at.sum())
            if cnt == 0:
                continue
            stats[n, c, :3] = [lab[n, v][at].mean() for v in range(3)]
            stats[n, c, 3:5] = ys[at].mean(), xs[at].mean()
            stats[n, c, 5] = cnt
            stats[n, c, 6] = float((ys[at] == 0).any() or (ys[at] == h - 1).any() or (xs[at] == 0).any() or (xs[at] == w - 1).any())
        for p, q in ((lv[n, :, :-1], lv[n, :, 1:]), (lv[n, :-1], lv[n, 1:])):
            e = (p >= 0) & (q >= 0) & (p != q)
            adj[n, p[e], q[e]] = 1
            adj[n, q[e], p[e]] = 1
    return stats, adj


def weights64(stats, adj):
    stats = np.asarray(stats, dtype=np.float64)
    b, k, _ = stats.shape
    out = np.full((b, k, k), np.inf)
    for n in range(b):
        act, bnd = stats[n, :, 5] > 0, stats[n, :, 6] > 0
        for i in range(k):
            for j in range(k):
                if i == j:
                    out[n, i, j] = 0.0
                elif act[i] and act[j] and (adj[n, i, j] or (bnd[i] and bnd[j])):
                    out[n, i, j] = math.sqrt(sum((stats[n, i, v] - stats[n, j, v]) ** 2 for v in range(3)))
    return out


def geodesic64(wgt):
    """Floyd-Warshall, pivot by pivot"""
    g = np.array(wgt, dtype=np.float64)
    for n in range(g.shape[0]):
        for k in range(g.shape[1]):
            g[n] = np.minimum(g[n], g[n][:, k:k + 1] + g[n][k:k + 1, :])
    return g


def background64(g, stats, sigma_clr=SIGMA_CLR, sigma_bndcon=SIGMA_BNDCON):
    g, stats = np.asarray(g, dtype=np.float64), np.asarray(stats, dtype=np.float64)
    b, k, _ = g.shape
    out = np.zeros((b, k))
    for n in range(b):
        act, bnd = stats[n, :, 5] > 0, stats[n, :, 6] > 0
        for i in np.flatnonzero(act):
            e = np.exp(-g[n, i, act] ** 2 / (2 * sigma_clr ** 2))
            area, length = e.sum(), e[bnd[act]].sum()
            out[n, i] = 1.0 - math.exp(-(length / math.sqrt(area)) ** 2 / (2 * sigma_bndcon ** 2))
    return out


def contrast64(g, stats, w_bg, h, w, sigma_spa=SIGMA_SPA):
    g, stats, w_bg = (np.asarray(v, dtype=np.float64) for v in (g, stats, w_bg))
    b, k, _ = g.shape
    out = np.zeros((b, k))
    for n in range(b):
        act = np.flatnonzero(stats[n, :, 5] > 0)
        for i in act:
            d = np.hypot(stats[n, i, 3] - stats[n, act, 3], stats[n, i, 4] - stats[n, act, 4]) / math.sqrt(h * h + w * w)
            out[n, i] = (g[n, i, act] * np.exp(-d ** 2 / (2 * sigma_spa ** 2)) * w_bg[n, act]).sum()
    return out


def unit_range64(v, act):
    out = np.zeros_like(v)
    if act.any() and v[act].max() > v[act].min():
        out[act] = (v[act] - v[act].min()) / (v[act].max() - v[act].min())
    return out


def system64(g, stats, adj, w_bg, wctr, sigma_clr=SIGMA_CLR, mu=MU):
    """-> per image (A, rhs, active indices, wCtr normalised): the system over the active clusters only"""
    g, stats, w_bg, wctr = (np.asarray(v, dtype=np.float64) for v in (g, stats, w_bg, wctr))
    out = []
    for n in range(g.shape[0]):
        act = stats[n, :, 5] > 0
        ix = np.flatnonzero(act)
        wn = unit_range64(wctr[n], act)
        s = np.asarray(adj[n])[np.ix_(ix, ix)].astype(np.float64) * (np.exp(-g[n][np.ix_(ix, ix)] ** 2 / (2 * sigma_clr ** 2)) + mu)
        a = np.diag(2 * w_bg[n, ix] + 2 * wn[ix] + 2 * s.sum(axis=1)) - 2 * s
        out.append((a, 2 * wn[ix], ix, wn))
    return out


def solve64(g, stats, adj, w_bg, wctr, sigma_clr=SIGMA_CLR, mu=MU):
    """-> (wCtr normalised, x, x normalised), each (B, K), 0 at inactive clusters"""
    stats = np.asarray(stats, dtype=np.float64)
    b, k, _ = stats.shape
    wn, x, xn = np.zeros((b, k)), np.zeros((b, k)), np.zeros((b, k))
    for n, (a, rhs, ix, wn_n) in enumerate(system64(g, stats, adj, w_bg, wctr, sigma_clr, mu)):
        wn[n] = wn_n
        x[n, ix] = np.linalg.solve(a, rhs)
        xn[n] = unit_range64(x[n], stats[n, :, 5] > 0)
    return wn, x, xn


def paint64(xnorm, labels, gy, gx):
    lv = valid_labels(labels, gy, gx)
    xnorm = np.asarray(xnorm, dtype=np.float64)
    out = np.zeros(lv.shape)
    for n in range(lv.shape[0]):
        out[n] = np.where(lv[n] >= 0, xnorm[n][np.maximum(lv[n], 0)], 0.0)
    return out


def rbd64(lab, labels, gy, gx, sigma_clr=SIGMA_CLR, sigma_bndcon=SIGMA_BNDCON, sigma_spa=SIGMA_SPA, mu=MU):
    """the whole definition in float64 -> dict of every stage's output and the map `sal`"""
    h, w = np.asarray(lab).shape[2:]
    stats, adj = region64(lab, labels, gy, gx)
    wgt = weights64(stats, adj)
    g = geodesic64(wgt)
    w_bg = background64(g, stats, sigma_clr, sigma_bndcon)
    wctr = contrast64(g, stats, w_bg, h, w, sigma_spa)
    wn, x, xn = solve64(g, stats, adj, w_bg, wctr, sigma_clr, mu)
    return dict(stats=stats, adj=adj, weights=wgt, geodesic=g, w_bg=w_bg, wctr=wctr, wctr_norm=wn, x=x, xnorm=xn,
                sal=paint64(xn, labels, gy, gx))


# ------------------------------------------------------------------------------------------------------------------------ the cases
#            name            H   W   gy  gx  content     B  a cluster to empty in image 0
CASES = {
    "blobs_emptied":      (48, 64, 6, 8, "blobs", 3, 19),
    "noise":              (48, 64, 6, 8, "noise", 2, None),
    "all_boundary":       (32, 32, 2, 3, "blobs", 2, None),
    "one_row_of_cells":   (40, 56, 1, 7, "blobs", 2, None),
    "disc":               (64, 64, 8, 8, "disc", 2, None),
    "k144_ragged_tiles":  (96, 96, 12, 12, "blobs", 2, None),
    "k81_tile_plus_17":   (80, 80, 9, 9, "noise", 2, None),
    "constant":           (40, 48, 5, 6, "constant", 2, None),
}

# beyond the table above: K = 576 > 512, nine tiles a side -- the second trip of every strided loop over the clusters (the row passes
# stride by 256, the solve by 512).  Kept out of CASES so that only the test that needs it pays for its restatement.
EXTRA = {
    "k576_second_trips": (96, 96, 24, 24, "noise", 2, 300),
}


def jittered_labels(h, w, gy, gx, rng):
    """a label map whose segments are the grid's cells with wavy borders: every pixel gets a cell of the 3 x 3 around its home cell"""
    hi, hj = (np.arange(h) * gy) // h, (np.arange(w) * gx) // w
    yy, xx = np.mgrid[:h, :w]
    ph, fr = rng.uniform(0, 2 * np.pi, 4), rng.uniform(1.5, 4.0, 4)
    u = np.sin(2 * np.pi * fr[0] * yy / h + ph[0]) + np.sin(2 * np.pi * fr[1] * xx / w + ph[1])
    v = np.sin(2 * np.pi * fr[2] * yy / h + ph[2]) + np.sin(2 * np.pi * fr[3] * xx / w + ph[3])
    di, dj = np.where(u > 1.0, 1, np.where(u < -1.0, -1, 0)), np.where(v > 1.0, 1, np.where(v < -1.0, -1, 0))
    return (np.clip(hi[:, None] + di, 0, gy - 1) * gx + np.clip(hj[None, :] + dj, 0, gx - 1)).astype(np.int32)


def empty_cluster(labels, k, gy, gx):
    """the pixels of cluster k go to their home cell's cluster, or, where that is k, to a cluster beside it in the row"""
    h, w = labels.shape
    home = ((np.arange(h) * gy) // h)[:, None] * gx + ((np.arange(w) * gx) // w)[None, :]
    beside = k + 1 if (k % gx) + 1 < gx else k - 1
    out = labels.copy()
    at = labels == k
    out[at] = np.where(home[at] != k, home[at], beside)
    return out


def synthetic_lab(h, w, content, rng):
    """a planar Lab image (3, H, W) float32: L in [0, 100], a and b in [-50, 50]"""
    yy, xx = np.mgrid[:h, :w].astype(np.float64)
    if content == "constant":                                # integers: every cluster mean is exact in float32, so all G = 0
        return np.broadcast_to(np.array([50.0, 8.0, -16.0], dtype=np.float32)[:, None, None], (3, h, w)).copy()
    if content == "noise":
        lab = np.stack([rng.uniform(0, 100, (h, w)), rng.uniform(-50, 50, (h, w)), rng.uniform(-50, 50, (h, w))])
    elif content == "disc":
        inside = (yy - h * rng.uniform(0.4, 0.6)) ** 2 + (xx - w * rng.uniform(0.4, 0.6)) ** 2 < (0.28 * min(h, w)) ** 2
        lab = np.where(inside[None], np.array([70.0, 20.0, 30.0])[:, None, None], np.array([30.0, -10.0, -20.0])[:, None, None])
        lab = lab + rng.normal(0, 0.5, (3, h, w))
    else:                                                    # blobs
        lab = np.stack([np.full((h, w), 40.0), np.zeros((h, w)), np.zeros((h, w))])
        for _ in range(4):
            cy, cx, r = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w, rng.uniform(0.1, 0.25) * min(h, w)
            bump = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * r * r))
            lab = lab + bump[None] * rng.uniform(-40, 40, 3)[:, None, None]
        lab = lab + rng.normal(0, 1.0, (3, h, w))
    return lab.astype(np.float32)


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (lab float32 (B, 3, H, W), labels int32 (B, H, W), (gy, gx)); the images of a batch differ"""
    h, w, gy, gx, content, b, emptied = CASES[name] if name in CASES else EXTRA[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100 if name in CASES else 1000 + sorted(EXTRA).index(name))
    lab = np.stack([synthetic_lab(h, w, content, rng) for _ in range(b)])
    labels = np.stack([jittered_labels(h, w, gy, gx, rng) for _ in range(b)])
    if emptied is not None:
        labels[0] = empty_cluster(labels[0], emptied, gy, gx)
    assert (valid_labels(labels, gy, gx) == labels).all()
    lab.setflags(write=False), labels.setflags(write=False)
    return lab, labels, (gy, gx)


@functools.lru_cache(maxsize=None)
def reference(name):
    """rbd64 of the case, made once and shared; treat it as read-only"""
    lab, labels, (gy, gx) = make(name)
    return rbd64(lab, labels, gy, gx)


def k_active(stats):
    """the largest number of active clusters among the images"""
    return int((np.asarray(stats)[..., 5] > 0).sum(axis=1).max())
