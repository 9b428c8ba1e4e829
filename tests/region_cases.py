"""The definition of include/vqseg.h's connected regions, restated as a plain Python / numpy union-find, and the case table of the
region suites (tests/test_regions_cpu.py, tests/test_regions_kernel_gpu.py and the predict / trainer suites).  Nothing of vq_seg_amd
is imported here.

    roots(values, connectivity, ignore)        (B, H, W) int32: the smallest row-major index of the pixel's region, -1 where ignored
    ids(roots)                                 ((B, H, W) int32 ranks by rising root, (B,) int32 counts); an entry outside [0, H W) is ignored
    areas(roots)                               (B, H, W) int32: the area at the root index, 0 elsewhere
    table(values, roots, ids, capacity)        ((B, capacity, 8) int32, (B, capacity, 2) int64)
    filter(values, roots, areas, min_area, fill)

All of it is integer arithmetic: every comparison against it is exact."""
import functools

import numpy as np

SHAPES = [(1, 1), (2, 2), (1, 70), (70, 1), (33, 65), (67, 131), (130, 130)]
BATCH_SHAPE = (3, 40, 72)
IGNORE = (255,)


def _find(parent, i):
    while parent[i] != i:
        parent[i] = parent[parent[i]]
        i = parent[i]
    return i


def roots_image(v, connectivity=4, ignore=()):
    """one image (H, W) -> (H, W) int32"""
    h, w = v.shape
    flat = [int(x) for x in v.reshape(-1)]
    ign = set(int(i) for i in ignore)
    parent = list(range(h * w))
    links = ((0, -1), (-1, 0)) + (((-1, -1), (-1, 1)) if connectivity == 8 else ())
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if flat[i] in ign:
                continue
            for dy, dx in links:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and flat[yy * w + xx] == flat[i]:
                    a, b = _find(parent, i), _find(parent, yy * w + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)           # the smaller index stays the root
    out = np.empty(h * w, dtype=np.int32)
    for i in range(h * w):
        out[i] = -1 if flat[i] in ign else _find(parent, i)
    return out.reshape(h, w)


def roots(values, connectivity=4, ignore=()):
    assert connectivity in (4, 8)
    return np.stack([roots_image(v, connectivity, ignore) for v in values])


def ids(root):
    b, h, w = root.shape
    n = h * w
    out = np.full((b, n), -1, dtype=np.int32)
    counts = np.zeros(b, dtype=np.int32)
    for k in range(b):
        r = root[k].reshape(-1).astype(np.int64)
        ok = (r >= 0) & (r < n)
        is_root = ok & (r == np.arange(n))
        rank = np.cumsum(is_root) - 1
        member = ok.copy()
        member[ok] = is_root[r[ok]]                             # a pixel whose entry does not point at a root belongs to no region
        out[k, member] = rank[r[member]]
        counts[k] = int(is_root.sum())
    return out.reshape(b, h, w), counts


def areas(root):
    b, h, w = root.shape
    n = h * w
    out = np.zeros((b, n), dtype=np.int32)
    for k in range(b):
        r = root[k].reshape(-1).astype(np.int64)
        r = r[(r >= 0) & (r < n)]
        out[k] = np.bincount(r, minlength=n).astype(np.int32)
    return out.reshape(b, h, w)


def table(values, root, id_, capacity):
    b, h, w = root.shape
    n = h * w
    tab = np.zeros((b, capacity, 8), dtype=np.int32)
    mom = np.zeros((b, capacity, 2), dtype=np.int64)
    ys, xs = np.divmod(np.arange(n), w)
    big = np.iinfo(np.int32).max
    for k in range(b):
        r, l, v = root[k].reshape(-1).astype(np.int64), id_[k].reshape(-1).astype(np.int64), values[k].reshape(-1)
        at = np.nonzero((r >= 0) & (r < n) & (l >= 0) & (l < capacity))[0]          # the pixels that have a row
        rows = l[at]
        t = np.zeros((capacity, 8), dtype=np.int64)
        t[:, (2, 3, 6)] = big
        np.add.at(t[:, 1], rows, 1)
        np.minimum.at(t[:, 2], rows, ys[at])
        np.minimum.at(t[:, 3], rows, xs[at])
        np.maximum.at(t[:, 4], rows, ys[at])
        np.maximum.at(t[:, 5], rows, xs[at])
        np.minimum.at(t[:, 6], rows, r[at])
        np.add.at(mom[k, :, 0], rows, ys[at])
        np.add.at(mom[k, :, 1], rows, xs[at])
        used = t[:, 1] > 0
        t[used, 0] = v[t[used, 6]]                                                   # the value at the root
        t[~used] = 0
        tab[k] = t
    return tab, mom


def filter(values, root, area, min_area, fill):                  # noqa: A001  (the definition's own word)
    """fill: an integer, or "neighbour" """
    b, h, w = root.shape
    n = h * w
    v, r, a = values.reshape(b, n), root.reshape(b, n).astype(np.int64), area.reshape(b, n)
    ok = (r >= 0) & (r < n)
    rs = np.where(ok, r, 0)
    small = ok & (np.take_along_axis(a, rs, axis=1) < min_area)
    if not isinstance(fill, str):
        return np.where(small, np.asarray(fill).astype(values.dtype), v).reshape(b, h, w)
    assert fill == "neighbour"
    ry, rx = np.divmod(rs, w)
    own = np.broadcast_to(np.arange(n), (b, n))
    src = np.where(rx > 0, rs - 1, np.where(ry > 0, rs - w, own))     # the pixel before the root: to its left, else above it, else none
    return np.where(small, np.take_along_axis(v, src, axis=1), v).reshape(b, h, w)


def remove_small(values, min_area, connectivity=4, ignore=(), fill=0):
    r = roots(values, connectivity, ignore)
    return filter(values, r, areas(r), min_area, fill)


# ------------------------------------------------------------------------------------------------------------------------------
# patterns: (H, W) uint8 maps with values in {0, 1, 2} and 255
# ------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([0x5EED] + [int(k) for k in key])


def random3(h, w, density, seed):
    """class 1 with probability `density`, the rest split between 0 and 2, 2 % of the pixels 255"""
    g = _rng(h, w, int(density * 100), seed)
    u = g.random((h, w))
    v = np.where(u < density, 1, np.where(u < density + (1 - density) / 2, 0, 2)).astype(np.uint8)
    v[g.random((h, w)) < 0.02] = 255
    return v


def constant(h, w):
    return np.full((h, w), 1, dtype=np.uint8)


def all_ignored(h, w):
    return np.full((h, w), 255, dtype=np.uint8)


def checkerboard(h, w):
    return ((np.arange(h)[:, None] + np.arange(w)[None, :]) % 2).astype(np.uint8)


def hstripes(h, w):
    return np.broadcast_to((np.arange(h) % 2).astype(np.uint8)[:, None], (h, w)).copy()


def vstripes(h, w):
    return np.broadcast_to((np.arange(w) % 2).astype(np.uint8)[None, :], (h, w)).copy()


def serpentine(h, w):
    """rows 0, 2, 4, .. of 1, joined alternately at the right and the left end: one region of 1 that runs through the whole image"""
    v = np.zeros((h, w), dtype=np.uint8)
    v[0::2] = 1
    for k, y in enumerate(range(1, h, 2)):
        if y + 1 < h:
            v[y, w - 1 if k % 2 == 0 else 0] = 1
    return v


def spiral(h, w):
    """a one-pixel path of 1 that winds inwards with a one-pixel gap: one region whose chain runs through the whole image"""
    v = np.zeros((h, w), dtype=np.uint8)

    def free(y, x):
        return not (0 <= y < h and 0 <= x < w) or v[y, x] == 0

    y, x, dy, dx = 0, 0, 0, 1
    v[0, 0] = 1
    while True:
        for _ in range(2):                                      # straight on, else one turn to the right, else the path ends
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and v[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return v
        y, x = ny, nx
        v[y, x] = 1


def diagonal(h, w):
    v = np.zeros((h, w), dtype=np.uint8)
    n = min(h, w)
    v[np.arange(n), np.arange(n)] = 1
    return v


def antidiagonal(h, w):
    v = np.zeros((h, w), dtype=np.uint8)
    n = min(h, w)
    v[np.arange(n), w - 1 - np.arange(n)] = 1
    return v


def rings(h, w):
    d = np.minimum(np.minimum(np.arange(h)[:, None], h - 1 - np.arange(h)[:, None]), np.minimum(np.arange(w)[None, :], w - 1 - np.arange(w)[None, :]))
    return (d % 3).astype(np.uint8)


def comb(h, w):
    """a spine along the top row and a tooth in every second column"""
    v = np.zeros((h, w), dtype=np.uint8)
    v[0] = 2
    v[:, 0::2] = 2
    if h > 1:
        v[-1] = 0
    return v


PATTERNS = {
    "random41": lambda h, w: random3(h, w, 0.41, 1),
    "random50": lambda h, w: random3(h, w, 0.50, 2),
    "random59": lambda h, w: random3(h, w, 0.59, 3),
    "constant": constant,
    "ignored": all_ignored,
    "checkerboard": checkerboard,
    "hstripes": hstripes,
    "vstripes": vstripes,
    "serpentine": serpentine,
    "spiral": spiral,
    "diagonal": diagonal,
    "antidiagonal": antidiagonal,
    "rings": rings,
    "comb": comb,
}


def batch_case():
    """3 x (40 x 72), different content per image; image 0's last row and image 1's first row carry the same value"""
    h, w = BATCH_SHAPE[1:]
    a, b, c = random3(h, w, 0.59, 11), random3(h, w, 0.41, 12), rings(h, w)
    a[-1] = 1
    b[0] = 1
    return np.stack([a, b, c])


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (1 or 3, H, W) uint8, read-only"""
    if name == "batch":
        v = batch_case()
    else:
        pattern, shape = name.rsplit("-", 1)
        h, w = (int(s) for s in shape.split("x"))
        v = PATTERNS[pattern](h, w)[None]
    v = np.ascontiguousarray(v, dtype=np.uint8)
    v.setflags(write=False)
    return v


CASES = [f"{p}-{h}x{w}" for p in PATTERNS for h, w in SHAPES] + ["batch"]
MIN_AREA = 5                                                    # of the filter checks: above the specks of the random maps, below the stripes
CAPACITY = 4096                                                 # rows of the table checks: the checkerboard of 130 x 130 overflows it


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """everything the definition gives for a case, computed once and shared (read-only arrays)"""
    v = case(name)
    r = roots(v, connectivity, IGNORE)
    i, c = ids(r)
    a = areas(r)
    t, m = table(v, r, i, CAPACITY)
    out = dict(values=v, roots=r, ids=i, counts=c, areas=a, table=t, moments=m,
               fill0=filter(v, r, a, MIN_AREA, 0), neighbour=filter(v, r, a, MIN_AREA, "neighbour"))
    for x in out.values():
        x.setflags(write=False)
    return out
