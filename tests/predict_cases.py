"""Shared by the prediction-path tests (vqseg_resize_argmax_f, nnf.resize_argmax, vq_seg_amd.predict): the shapes, the input makers
and the restatement of the operation with plain torch ops, written out here on its own (it does not call the package):

    acc   = sum over views, in order, of resize(view.flip(dims of its code), size);   acc = acc * (1 / V) if V > 1
    label = acc.argmax(1);   top = softmax(acc, 1).max(1);   counts = bincount(C * target + label) per image over targets in [0, C)

Shapes: the smallest at which the kernel can still go wrong (a wave takes 256 consecutive output pixels of one image, a workgroup 1024, and
packs the labels of a whole, 4-byte aligned run into words)."""
import functools

import torch
import torch.nn.functional as F

# (b, c, h, w) -> (ho, wo)
SHAPES = [
    ((3, 2, 5, 7), (13, 9)),          # non-integer up-scaling; 117 pixels per image: images at offsets that are no multiple of 4
    ((3, 3, 12, 16), (7, 5)),         # down-scaling
    ((1, 4, 8, 8), (8, 8)),           # identity size
    ((2, 3, 1, 6), (4, 17)),          # a one-row source
    ((2, 3, 9, 11), (16, 16)),        # 256 output pixels
    ((2, 3, 9, 11), (15, 17)),        # 255: a partial label pack
    ((2, 3, 9, 11), (1, 257)),        # 257: one past a wave's 256 pixels (a whole run, then a one-pixel run), a one-row output
    ((3, 3, 16, 16), (31, 33)),       # odd output sizes
]
GRID_STRIDE = ((3, 3, 64, 64), (300, 300))     # 264 tiles under nn_grid_cap = 256: the grid-stride loop
IDS = ["x".join(map(str, s)) + "-" + "x".join(map(str, o)) for s, o in SHAPES]
LAYOUTS = ["nchw", "channels_last"]
FLIP_DIMS = {0: (), 1: (3,), 2: (2,), 3: (2, 3)}             # bit 0 flips columns, bit 1 rows
LOGIT_ERR = 1.4e-5                                           # what fp32 F.interpolate itself deviates from fp64 on the N(0, 4^2) inputs (small shapes)
GAP = 1e-4                                                   # labels are compared where the fp64 top-two logit gap exceeds this (7 x LOGIT_ERR)
U = 2.0 ** -24


def lay(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else t.contiguous()


@functools.lru_cache(maxsize=None)
def logits(shape, seed=0, kind="normal"):
    """CPU float32 (b, c, h, w).  "normal": N(0, 4^2);  "ties": the same quantised to multiples of 0.5, so that interpolated ties occur, with
    class 1 of image 0 a copy of its class 0 (a tie at every pixel), and the first maximum must win;  "special": a NaN, +inf and -inf
    planted in each image.  The result is shared: do not modify it."""
    g = torch.Generator().manual_seed(1000 * seed + sum(shape) + 7 * shape[1])
    z = torch.randn(shape, generator=g) * 4.0
    if kind == "ties":
        z = torch.round(z * 2.0) / 2.0
        z[0, 1] = z[0, 0]                                    # image 0: classes 0 and 1 tie at every pixel, at any size
    elif kind == "special":
        b, c, h, w = shape
        flat = z.reshape(b, -1)
        n = flat.shape[1]
        for i in range(b):
            at = torch.randperm(n, generator=g)[:3]
            flat[i, at[0]] = float("nan")
            flat[i, at[1]] = float("inf")
            flat[i, at[2]] = float("-inf")
    elif kind != "normal":
        raise ValueError(kind)
    return z


@functools.lru_cache(maxsize=None)
def targets(shape, size, seed=0, dtype=torch.int64):
    """CPU (b, ho, wo) integer labels: valid classes with 255 (the ignore value) and an out-of-range 7 among them"""
    b, c = shape[:2]
    g = torch.Generator().manual_seed(77 + 1000 * seed + sum(shape) + size[0] * 31 + size[1])
    t = torch.randint(0, c, (b,) + tuple(size), generator=g)
    r = torch.rand((b,) + tuple(size), generator=g)
    t[r < 0.10] = 255
    t[(r >= 0.10) & (r < 0.15)] = 7
    return t.to(dtype)


def accumulate(views, flips, size, dtype=None):
    """the mean logits at `size`: sum over the views in order of resize(view.flip(dims)), times 1 / V when V > 1 (torch ops, the views'
    device; `dtype` float64 for the independent reference)"""
    acc = None
    for v, f in zip(views, flips):
        v = v if dtype is None else v.to(dtype)
        v = v.flip(FLIP_DIMS[f]) if f else v
        r = F.interpolate(v, size=tuple(size), mode="bilinear", align_corners=False)
        acc = r if acc is None else acc + r
    return acc * (1.0 / len(views)) if len(views) > 1 else acc


def confusion(label, target, c):
    """(b, c, c) int64: bincount of c * target + label per image over the targets in [0, c), rows = ground truth"""
    b = label.shape[0]
    out = torch.zeros((b, c, c), dtype=torch.int64)
    for i in range(b):
        t, p = target[i].reshape(-1).long().cpu(), label[i].reshape(-1).long().cpu()
        keep = (t >= 0) & (t < c)
        out[i] = torch.bincount(c * t[keep] + p[keep], minlength=c * c).reshape(c, c)
    return out


def restatement(views, flips, size, target=None, dtype=None):
    """-> (acc, label int64, top, counts | None) with torch ops"""
    acc = accumulate(views, flips, size, dtype)
    label = acc.argmax(dim=1)
    top = torch.softmax(acc, dim=1).max(dim=1).values
    counts = confusion(label, target, acc.shape[1]) if target is not None else None
    return acc, label, top, counts


def top_tolerance(acc64, logit_err=LOGIT_ERR):
    """bound on |top - fp64 softmax maximum| per pixel.  tests/test_loss_kernels_gpu.py allows softmax_stats' top probability
    u top (share + (C - 1) + 1), share = sum_c p_c (|z_c - max| + 2), against the fp64 softmax of the SAME logits; here the logits
    themselves carry `logit_err` (fp32 interpolation against fp64), and sum_c |d top / d z_c| = 2 top (1 - top) <= 1 / 2."""
    c = acc64.shape[1]
    p = torch.softmax(acc64, dim=1)
    d = (acc64 - acc64.amax(dim=1, keepdim=True)).abs()
    share = (p * (d + 2)).sum(dim=1)
    return U * p.amax(dim=1) * (share + c) + 0.5 * logit_err


class Stub(torch.nn.Module):
    """a plain torch 1 x 1 convolution that returns (logits, extra), as the package's networks do; counts its calls and remembers
    whether it ran in eval mode"""

    def __init__(self, num_classes=3, seed=0, pool=1):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, num_classes, 1, bias=True)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 3.0)
            self.conv.bias.copy_(torch.randn(self.conv.bias.shape, generator=g))
        self.pool, self.seen = pool, []

    def forward(self, x):
        self.seen.append((self.training, x.detach().clone()))
        y = self.conv(x)
        if self.pool > 1:
            y = F.avg_pool2d(y, self.pool)
        return y, torch.zeros(1)
