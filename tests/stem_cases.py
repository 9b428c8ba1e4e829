"""Shapes, operands, fp64 references and acceptance bounds of the stem and reflect-fold parity tests
(tests/test_stem_kernels_gpu.py; tests/test_stem_bound_cpu.py checks the bounds themselves without a GPU).

Four kernel families: the fused stem (vqseg_stem7_conv_f), the stem's patch matrices (vqseg_im2col_f), the gradient fold of reflect
padding 1 (vqseg_reflect_fold_f) and the border-ring form of the same fold (vqseg_reflect_ring_f).  Every reference is computed once
per case in float64 from the values the kernel receives and shared; nobody writes into one.  No bound has a term taken from the
kernels' output: each is the arithmetic of the operation (products of bf16 values are exact in fp32; an fp32 accumulation of K terms
errs by at most K 2^-23 S with S the sum of the terms' magnitudes; a rounding to bf16 is within 2^-8 relative, 2^-9 when to nearest).
Measured figures: profiles/stem_parity.md."""
import functools

import torch
import torch.nn.functional as F

from tests import synth
from tests.dispatch_cases import bound

U = 2.0 ** -24                                               # unit roundoff of fp32

# ---------------------------------------------------------------------------------------------------------------------------
# A. the fused stem: 7x7 / stride 2 / pad 3, 3 -> 64 channels, straight from the fp32 image; 128 output pixels of a row per workgroup
# ---------------------------------------------------------------------------------------------------------------------------
STEM_CASES = {
    # name -> n, h, w (each runs with zero and with reflect padding)
    "S1": (1, 4, 256),          # the smallest accepted image: ho = 2, both reflections land in the same seven staged rows; one strip
    "S2": (2, 5, 255),          # odd extents: the right-border reflection 2W - 2 - iw, one more zero column; image 1 checks the stride
    "S3": (1, 7, 512),          # two strips: strip 1's left halo is image, not padding
    "S4": (1, 6, 768),          # three strips: the middle one has no padding on either side
}
STEM_K = 176                                                 # eleven K steps of 16: padded positions meet zero weights (exact zeros)
STEM_COUT = 64


def stem_out_size(h, w):
    return (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1


def _stem_seed(case):
    return 3000 + 23 * sorted(STEM_CASES).index(case)


@functools.lru_cache(maxsize=None)
def stem_operands(case):
    """x [n, h, w, 3] fp32 (NOT bf16-exact: the kernel's own rounding is part of the test), w [64, 3, 7, 7] fp32"""
    n, h, w = STEM_CASES[case]
    x = synth.uniform(_stem_seed(case), (n, h, w, 3), -2.2, 2.7)
    wt = synth.uniform(_stem_seed(case) + 1, (STEM_COUT, 3, 7, 7), -1, 1) * (2.0 / 147) ** 0.5
    return x, wt


def split(v):
    """fp32 -> (hi, lo) fp32 tensors holding bf16 values: hi = bf16(v), lo = bf16(v - hi)"""
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def stem_weight_image(wt, s3):
    """The image vqseg.h documents: [64][176] bf16, column kh * 24 + kw * 3 + ci = bf16(w[co][ci][kh][kw]), zero elsewhere;
    split-3: [64][2][176] = the hi image | the image of bf16(w - hi)."""
    cout = wt.shape[0]
    img = torch.zeros(cout, 7, 24, dtype=torch.float32)
    img[:, :, :21] = wt.permute(0, 2, 3, 1).reshape(cout, 7, 21)                     # [co][kh][(kw, ci)]
    img = torch.cat([img.reshape(cout, 168), torch.zeros(cout, 8)], 1)
    hi, lo = split(img)
    return (torch.stack([hi, lo], 1) if s3 else hi).bfloat16().contiguous()


def stem_patches(x, reflect, right_reflect_off_by_one=False):
    """[n * ho * wo, 147] patch rows of x [n, h, w, 3] (any float dtype), columns (kh, kw, ci).  right_reflect_off_by_one: the
    mutation of test_stem_bound_cpu -- columns right of the image read 2W - 1 - iw instead of 2W - 2 - iw."""
    n, h, w, c = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (3, 3, 3, 3), mode="reflect" if reflect else "constant")
    if right_reflect_off_by_one:
        assert reflect
        xp = xp.clone()
        for j in range(3):                                   # padded column 3 + w + j holds iw = w + j -> image column 2w - 1 - iw
            xp[..., 3 + w + j] = xp[..., 3 + (w - 1 - j)]
    cols = F.unfold(xp, 7, stride=2)                         # [n, (ci, kh, kw), ho * wo]
    return cols.reshape(n, c, 7, 7, -1).permute(0, 4, 2, 3, 1).reshape(-1, 147)


def stem_weight_matrix(wt):
    """[147, 64], rows (kh, kw, ci) as stem_patches' columns"""
    return wt.permute(0, 2, 3, 1).reshape(wt.shape[0], 147).t()


@functools.lru_cache(maxsize=None)
def stem_reference(case, reflect):
    """dict of [M, 64] float64 matrices:
    ref, S      the convolution of bf16(x) with bf16(w), and the same of the absolute values
    ref3, S3    x_hi w_hi + x_lo w_hi + x_hi w_lo on the split operands, and the same of the absolute values
    true, St    the convolution of the unrounded fp32 operands, and the same of the absolute values"""
    x, wt = stem_operands(case)
    xh, xl = split(x)
    wh, wl = split(wt)
    p = lambda t: stem_patches(t.double(), reflect)
    b = lambda t: stem_weight_matrix(t.double())
    ph, pl, bh, bl = p(xh), p(xl), b(wh), b(wl)
    pt, bt = p(x), b(wt)
    return {
        "ref": ph @ bh, "S": ph.abs() @ bh.abs(),
        "ref3": ph @ bh + pl @ bh + ph @ bl, "S3": ph.abs() @ bh.abs() + pl.abs() @ bh.abs() + ph.abs() @ bl.abs(),
        "true": pt @ bt, "St": pt.abs() @ bt.abs(),
    }


def stem_affine():
    """(scale, shift) fp32 [64] of the fused epilogues: scale in (0.5, 1.5) with every third channel negated, shift in (-0.3, 0.3)"""
    scale = synth.uniform(3501, (STEM_COUT,), 0.5, 1.5)
    scale[::3] = -scale[::3]
    return scale, synth.uniform(3502, (STEM_COUT,), -0.3, 0.3)


def stem_raw_bound(r):
    """A.1, raw bf16 output: dispatch_cases.bound with K = 176"""
    return bound(r["ref"], r["S"], STEM_K)


def stem_affine_bound(r, scale, shift):
    """A.2, bf16 output of fma(acc, scale, shift) [+ ReLU]: (pre, bound) with pre = scale ref + shift and
    bound = 2^-8 |pre| + |scale| 176 2^-23 S + 2 2^-24 (|scale ref| + |shift|): the rounding to bf16, the accumulation error
    carried through the scale, the two fp32 roundings of the affine.  ReLU is 1-Lipschitz: max(pre, 0) under the same bound."""
    sc, sh = scale.double(), shift.double()
    pre = sc * r["ref"] + sh
    return pre, 2.0 ** -8 * pre.abs() + sc.abs() * STEM_K * 2.0 ** -23 * r["S"] + 2 * U * ((sc * r["ref"]).abs() + sh.abs())


def stem_s3_bound(r, scale, shift):
    """A.3, split-3 output v = hi + lo of relu(fma(acc, scale, shift)): (pre3, bound) with pre3 = scale ref3 + shift and
    bound = |scale| 3 176 2^-23 S3 + 2 2^-24 (|scale ref3| + |shift|) + 2^-17 |pre3|: three products per K column, the affine's
    two roundings, and the re-split (lo is rounded to 8 bits below hi's 8)."""
    sc, sh = scale.double(), shift.double()
    pre = sc * r["ref3"] + sh
    return pre, sc.abs() * 3 * STEM_K * 2.0 ** -23 * r["S3"] + 2 * U * ((sc * r["ref3"]).abs() + sh.abs()) + 2.0 ** -17 * pre.abs()


def outside(got, want, limit):
    """coordinates of the elements of `got` further than `limit` from `want` (NaN counts as outside)"""
    return (~((got.double() - want).abs() <= limit)).nonzero()


# ---------------------------------------------------------------------------------------------------------------------------
# B. vqseg_im2col_f: an exact operation, compared bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def im2col_out_size(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def im2col_reference(x, k, stride, pad, reflect, kp, form):
    """x [n, h, w, cin] fp32 -> the patch rows [M, kp] (form 0: fp32, 1: bf16) or [M, 2 kp] (form 2: hi | lo, bf16): F.unfold of the
    padded image, columns (kh, kw, ci), zero-extended to kp"""
    n, h, w, cin = x.shape
    xp = x.permute(0, 3, 1, 2)
    if pad:
        xp = F.pad(xp, (pad, pad, pad, pad), mode="reflect" if reflect else "constant")
    cols = F.unfold(xp, k, stride=stride).reshape(n, cin, k, k, -1).permute(0, 4, 2, 3, 1).reshape(-1, k * k * cin)
    v = torch.cat([cols, torch.zeros(cols.shape[0], kp - cols.shape[1])], 1)
    if form == 0:
        return v
    hi = v.bfloat16()
    return hi if form == 1 else torch.cat([hi, (v - hi.float()).bfloat16()], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# C. vqseg_reflect_fold_f: gp [n, h + 2, w + 2, c] -> gx [n, h, w, c], the gradient of reflect padding 1
# ---------------------------------------------------------------------------------------------------------------------------
FOLD_CASES = [
    # n, h, w, c
    (2, 2, 2, 8),               # h = w = 2: row 0 gathers padded rows 1 and 3, row 1 rows 2 and 0
    (1, 3, 3, 8),               # the centre pixel is row 1 AND row h - 2: nine padded positions
    (2, 4, 5, 16),
    (1, 5, 4, 12),              # bf16: the scalar instantiation (12 % 8), fp32: four channels per thread
    (2, 3, 6, 5),               # scalar in both
    (1, 2, 7, 24),
]
# more than 256 x 256 threads' worth of work in both vector instantiations (129 * 131 * 32 / 8 = 67596): under nn_grid_cap = 256,
# the smallest value the option takes, every thread makes a second trip through the grid-stride loop
FOLD_WRAP_CASE = (1, 129, 131, 32)


def reflect_fold(gp):
    """gp [n, h + 2, w + 2, c] float64 -> [n, h, w, c]: autograd of F.pad(x, (1, 1, 1, 1), "reflect") with cotangent gp"""
    n, hp, wp, c = gp.shape
    x = torch.zeros(n, c, hp - 2, wp - 2, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.pad(x, (1, 1, 1, 1), mode="reflect"), x, gp.permute(0, 3, 1, 2))
    return g.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fold_reference(case, bf16):
    """(gp in the element type, ref, S, t): the fold of gp, of |gp| and of ones (terms per pixel), float64 [n, h, w, c]"""
    n, h, w, c = case
    gp = synth.uniform(4000 + 7 * h + 3 * w + c, (n, h + 2, w + 2, c), -1, 1)
    gp = gp.bfloat16() if bf16 else gp
    return gp, reflect_fold(gp.double()), reflect_fold(gp.double().abs()), reflect_fold(torch.ones(gp.shape, dtype=torch.float64))


def half_ulp_bf16(v):
    """half a bf16 ulp at magnitude |v| (the expression of tests/test_nn_kernels_gpu.py)"""
    _, e = torch.frexp(v.abs().double().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 9)


def sum_bound(ref, S, k, bf16):
    """The bound test_nn_kernels_gpu.check applies: k 2^-24 S, plus half a bf16 ulp at the magnitude the fp32 result can reach when
    the store is bf16.  k (a number or a tensor): fp32 roundings of the kernel's expression -- one per addition of a fold."""
    b = k * U * S.double()
    return b + half_ulp_bf16(ref.abs() + b) if bf16 else b


# ---------------------------------------------------------------------------------------------------------------------------
# D. vqseg_reflect_ring_f: the full correlation on the border ring of the padded grid, folded onto rows 1 / h-2, columns 1 / w-2
# ---------------------------------------------------------------------------------------------------------------------------
RING_CASES = {
    # name -> n, h, w, cgy, cgx, the LDS-DMA instantiation launch_conv_impl's ring branch takes (conv_internal.h: 0x1TBWUMf).
    # The branch picks the tile by bn = cgx >= 128 ? 128 : cgx >= 64 ? 64 : 32; 3x3 taps: the generic prologue (f bit 2 clear);
    # more than one chunk of bn channels (and at most conv_xcd_pair = 8): the XCD-pair grid (f bit 0).
    "R1": (1, 4, 4, 64, 8, 0x1114310),       # the smallest accepted shape: <128, 32, 4, 3>, one chunk with 8 of its 32 channels
    "R2": (2, 5, 7, 64, 72, 0x1124311),      # <128, 64, 4, 3>, two chunks, the second holds 8 channels
    "R3": (1, 4, 9, 128, 64, 0x1124310),     # two 64-channel K stages per tap; one chunk
    "R4": (2, 6, 4, 64, 136, 0x1144211),     # <128, 128, 4, 2>, two chunks, the second holds 8 channels
}


def ring_len(h, w):
    return 2 * (w + 2) + 2 * h


def border_of(p):
    """p [n, h + 2, w + 2, c] -> the ring [n, 2 (w + 2) + 2 h, c] in the documented order: top row, bottom row, left column and right
    column over padded rows 1 .. h"""
    return torch.cat([p[:, 0], p[:, -1], p[:, 1:-1, 0], p[:, 1:-1, -1]], 1)


def ring_to_padded(ring, h, w, swap_columns=False):
    """the inverse of border_of with a zero interior.  swap_columns: the mutation of test_stem_bound_cpu -- the left and right column
    segments of the ring exchanged."""
    n, _, c = ring.shape
    wp = w + 2
    p = torch.zeros(n, h + 2, wp, c, dtype=ring.dtype)
    p[:, 0], p[:, -1] = ring[:, :wp], ring[:, wp:2 * wp]
    left, right = ring[:, 2 * wp:2 * wp + h], ring[:, 2 * wp + h:]
    if swap_columns:
        left, right = right, left
    p[:, 1:-1, 0], p[:, 1:-1, -1] = left, right
    return p


def ring_fold_reference(g0, ring, h, w):
    """(expected, S, k) float64 [n, h, w, c]: g0 + the ring positions that reflect onto each pixel (the map of F.pad(.., "reflect")'s
    autograd, the padded grid's interior being zero), the same of the absolute values, and the number of added terms (0 .. 3)"""
    r = ring.double()
    return (g0.double() + reflect_fold(ring_to_padded(r, h, w)), g0.double().abs() + reflect_fold(ring_to_padded(r.abs(), h, w)),
            reflect_fold(ring_to_padded(torch.ones_like(r), h, w)))


def _ring_seed(case):
    return 5000 + 31 * sorted(RING_CASES).index(case)


@functools.lru_cache(maxsize=None)
def ring_operands(case):
    """gy [n, h, w, cgy] bf16, w [cgy, cgx, 3, 3] fp32 holding bf16 values, G0 [n, h, w, cgx] bf16 (what gx holds before the call)"""
    n, h, w, cgy, cgx, _id = RING_CASES[case]
    gy = synth.uniform(_ring_seed(case), (n, h, w, cgy), -1, 1).bfloat16()
    wt = (synth.uniform(_ring_seed(case) + 1, (cgy, cgx, 3, 3), -1, 1) * (2.0 / (9 * cgx)) ** 0.5).bfloat16().float()
    g0 = synth.uniform(_ring_seed(case) + 2, (n, h, w, cgx), -1, 1).bfloat16()
    return gy, wt, g0


@functools.lru_cache(maxsize=None)
def ring_reference(case):
    """(ref, S) [n, ring length, cgx] float64: the border of the gradient of F.conv2d(xp, w) with respect to the (h + 2) x (w + 2)
    input xp with cotangent gy, and of the same with |w| and |gy|"""
    n, h, w, cgy, cgx, _id = RING_CASES[case]
    gy, wt, _g0 = ring_operands(case)

    def full(g, wq):
        xp = torch.zeros(n, cgx, h + 2, w + 2, dtype=torch.float64, requires_grad=True)
        (gp,) = torch.autograd.grad(F.conv2d(xp, wq), xp, g.permute(0, 3, 1, 2))
        return border_of(gp.permute(0, 2, 3, 1))

    return full(gy.double(), wt.double()), full(gy.double().abs(), wt.double().abs())
