"""The dense-CRF contract (include/vqseg.h, vq_seg_amd/utils/crf.py) restated in float64 numpy with the (N, N) kernel matrices
written out, and the seeded cases the CRF tests share.

A case is a blocky image with Gaussian noise on it and noisy probabilities that agree with the blocks about 70 % of the time: the
refinement then changes a good share of the labels, so a kernel that does nothing fails.  `case` asserts on the CPU that after each
of the iterations tested every pixel's float64 top-two probability gap is at least MIN_GAP, so the label comparison of the GPU
tests excludes no pixel.  References are computed once per process and must be left unchanged."""
import functools
import math

import numpy as np

ITERS = (1, 2, 10)                                          # ping-pong parity: odd, even, the default count
MIN_GAP = 1e-4
DEFAULTS = dict(bi_w=7.0, bi_xy_std=50.0, bi_rgb_std=4.0, pos_w=3.0, pos_xy_std=3.0, truncate=4.0)
SETTINGS = {                                                # name -> keyword arguments of DenseCRF / nnf.dense_crf (without iter_max)
    "cut": dict(DEFAULTS, pos_xy_std=1.5, bi_xy_std=4.0, truncate=2.0),        # R = 3 and 8: inside the image, cut at every border
    "defaults": dict(DEFAULTS),                                                  # R = 12 and 200: the support is larger than the image
    "full": dict(DEFAULTS, truncate=None),
}
SHAPES = [(2, 3, 37, 53), (3, 2, 9, 13), (2, 4, 33, 20), (1, 3, 64, 64)]          # (B, C, H, W)
SEEDS = {(2, 3, 37, 53): 20, (3, 2, 9, 13): 12, (2, 4, 33, 20): 13, (1, 3, 64, 64): 22}       # picked so that `case` holds its gap


def restate(image, prob, iters, bi_w=7.0, bi_xy_std=50.0, bi_rgb_std=4.0, pos_w=3.0, pos_xy_std=3.0, truncate=4.0):
    """image (3, H, W) float32 in [0, 1], prob (C, H, W) -> {t: Q (C, H, W) float64 after t updates} for t in `iters` (0: Q0)"""
    c, h, w = prob.shape
    rgb = (np.clip(image.astype(np.float32), 0, 1) * np.float32(255)).astype(np.ubyte).astype(np.float64).reshape(3, -1).T
    u = -np.log(np.clip(prob.astype(np.float64), 1e-5, 1.0)).reshape(c, -1).T                     # (N, C)
    ys, xs = (g.reshape(-1).astype(np.float64) for g in np.mgrid[0:h, 0:w])
    dx, dy = np.abs(xs[:, None] - xs[None, :]), np.abs(ys[:, None] - ys[None, :])
    d2 = dx * dx + dy * dy
    c2 = sum((rgb[:, None, k] - rgb[None, :, k]) ** 2 for k in range(3))

    def support(xy_std):
        r = math.inf if truncate is None else math.ceil(truncate * xy_std)
        return (dx <= r) & (dy <= r)

    k_pos = np.exp(-0.5 * d2 / pos_xy_std ** 2) * support(pos_xy_std)
    k_bi = np.exp(-0.5 * (d2 / bi_xy_std ** 2 + c2 / bi_rgb_std ** 2)) * support(bi_xy_std)
    n_pos, n_bi = 1.0 / np.sqrt(k_pos.sum(axis=1) + 1e-20), 1.0 / np.sqrt(k_bi.sum(axis=1) + 1e-20)

    def softmax(e):
        z = np.exp(e - e.max(axis=1, keepdims=True))
        return z / z.sum(axis=1, keepdims=True)

    q, out = softmax(-u), {}
    for t in range(max(iters) + 1):
        if t in iters:
            out[t] = q.T.reshape(c, h, w).copy()
        e = -u + pos_w * (n_pos[:, None] * (k_pos @ (n_pos[:, None] * q))) + bi_w * (n_bi[:, None] * (k_bi @ (n_bi[:, None] * q)))
        q = softmax(e)
    return out


def make_inputs(seed, b, c, h, w):
    """-> images (B, 3, H, W) float32 in [0, 1], probs (B, C, H, W) float32 with rows that sum to 1; every image its own"""
    rng = np.random.default_rng(seed)
    images, probs = np.empty((b, 3, h, w), np.float32), np.empty((b, c, h, w), np.float32)
    for n in range(b):
        cell = int(rng.integers(4, 9))
        grid = rng.integers(0, c, size=(h // cell + 1, w // cell + 1))
        blocks = np.kron(grid, np.ones((cell, cell), dtype=np.int64))[:h, :w]                      # the blocky truth
        colours = rng.uniform(0.1, 0.9, size=(c, 3))
        images[n] = np.clip(colours[blocks].transpose(2, 0, 1) + rng.normal(0.0, 0.02, size=(3, h, w)), 0, 1)
        guess = np.where(rng.uniform(size=(h, w)) < 0.7, blocks, rng.integers(0, c, size=(h, w)))    # agrees about 70 % of the time
        logits = rng.normal(0.0, 0.5, size=(c, h, w)) + 1.2 * (np.arange(c)[:, None, None] == guess[None])
        z = np.exp(logits - logits.max(axis=0, keepdims=True))
        probs[n] = z / z.sum(axis=0, keepdims=True)
    return images, probs


@functools.lru_cache(maxsize=None)
def case(shape, setting):
    """-> (images, probs, {t: Q (B, C, H, W) float64}) for t in ITERS of SHAPES[...] under SETTINGS[setting]; asserts the gap"""
    b, c, h, w = shape
    images, probs = make_inputs(SEEDS[shape], b, c, h, w)
    per_image = [restate(images[n], probs[n], ITERS, **SETTINGS[setting]) for n in range(b)]
    ref = {t: np.stack([r[t] for r in per_image]) for t in ITERS}
    for t in ITERS:
        top2 = np.sort(ref[t], axis=1)[:, -2:]
        gap = float((top2[:, 1] - top2[:, 0]).min())
        assert gap >= MIN_GAP, f"case {shape} {setting}: top-two gap {gap:.3g} after {t} iterations; pick another seed"
    for a in (images, probs, *ref.values()):
        a.setflags(write=False)
    return images, probs, ref
