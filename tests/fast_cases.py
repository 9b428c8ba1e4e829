"""Shapes, operands, fp64 references, instantiation ids and a CPU emulation of the bf16 convolution kernels the training step
spends its time in: conv3x3_patch_kernel (forward with raw output + BatchNorm partials, fused affine epilogues, data-gradient form),
the 128-row conv_igemm_glds_kernel tiles with taps and strides, and the bf16 stride-2 data gradients (vqseg_conv2d_dgrad_s2_f on
parity classes, vqseg_conv2d_dgrad_s2_fold_f in one launch + reflect_s2_ring_add_kernel).  tests/test_fast_conv_gpu.py runs the
kernels against this; tests/test_fast_bound_cpu.py checks without a GPU that the bound passes the documented arithmetic and sees
the ways a tiled bf16 kernel goes wrong.

Every case is a GEMM  out[r, j] = sum_q A[r, q] B[q, j]  over bf16-exact operands, as in tests/precise_cases.py (A: the im2col matrix
of the launched convolution, columns (tap, channel); B: the weight image).  The reference is A B in fp64 next to S = |A| |B|, once per
geometry (cases that differ only in their options share it); nobody writes into them.

The acceptance bound is tests/dispatch_cases.bound, unchanged:  |y - ref| <= 2^-8 |ref| + K 2^-23 S  for every element, none
excluded; an element with S = 0 has a zero bound and must be exactly 0.  K: taps x channels of the launched convolution, per pixel
for the parity classes of a stride-2 data gradient (precise_cases.contraction's count)."""
import functools
import zlib

import torch
import torch.nn.functional as F

from tests import dispatch_cases as dc
from tests import precise_cases as pc
from tests import stem_cases
from tests import synth

U = 2.0 ** -23
PATCH = (("conv3x3_patch_min_workgroups", 1),)             # the patch kernel's grid bar lowered: what every A / B case runs under
TALL = PATCH + (("conv3x3_patch_tile512_min_workgroups", 1),)


# instantiation ids, conv_internal.h: conv_variant_patch / conv_variant_glds / conv_variant_igemm
def patch_id(bn, nbw, unroll, ck, tbm=256, pair=False):
    return 3 << 24 | tbm // 256 << 20 | bn // 32 << 16 | nbw << 12 | ck // 32 << 8 | int(unroll) << 4 | int(pair)


def glds_id(bn, nbuf, minw=1, cls=False, pair=False, tbm=128, nw=4):
    return 1 << 24 | tbm // 128 << 20 | bn // 32 << 16 | nw << 12 | nbuf << 8 | minw << 4 | int(cls) * 2 | int(pair)


def igemm_id(bn):
    return 2 << 24 | bn // 32 << 16 | 1 << 8


# name -> kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, options.  Geometry is the FORWARD layer's (x [n, h, w, c1 + c2] ->
# y [n, ho, wo, cout]); kind: "fwd", "dgrad" (data gradient as precise_cases: stride 1 zero padding on the input grid, stride 2 on
# the padded grid / k = 1 the input grid) or "fold" (vqseg_conv2d_dgrad_s2_fold_f: the unpadded gradient of a 3x3 stride-2 layer).
CASES = {
    # A. conv3x3_patch_kernel.  Tiles of 8 x 32 (W % 32 == 0) or 16 x 16 pixels, 512-pixel tiles 16 x 32 or 32 x 16; two tiles along
    # each axis of every geometry; n = 2 at least once per geometry (a halo row meets the next image)
    "P1": ("fwd", 2, 16, 64, 64, 64, 128, 3, 1, 1, False, PATCH),         # <128, 3, true>; 8 x 32; concat on a 64-channel boundary
    "P1u2": ("fwd", 2, 16, 64, 64, 64, 128, 3, 1, 1, False, PATCH + (("conv3x3_patch_unroll", 2),)),      # <128, 4, true>
    "P1u0": ("fwd", 2, 16, 64, 64, 64, 128, 3, 1, 1, False, PATCH + (("conv3x3_patch_unroll", 0),)),      # <128, 3, false>
    "P2": ("fwd", 1, 16, 64, 128, 64, 256, 3, 1, 1, True, PATCH),         # <256, 2, false>; 192 -> 256, reflect, concat
    "P2z": ("fwd", 1, 16, 64, 64, 0, 256, 3, 1, 1, False, PATCH),         # ... zero padding, one source (the bit-mask entry takes no other)
    "P3": ("fwd", 2, 32, 48, 64, 0, 384, 3, 1, 1, False, PATCH),          # <128, 3, true>, three Cout chunks; 16 x 16 tiles, 2 x 3 an image
    "P3r": ("fwd", 1, 32, 48, 128, 0, 128, 3, 1, 1, True, PATCH),         # ... 16 x 16 tiles with reflect padding
    "P5": ("fwd", 2, 16, 64, 64, 0, 64, 3, 1, 1, False, PATCH),           # <64, 3, true>
    "P5r": ("fwd", 2, 32, 48, 64, 0, 64, 3, 1, 1, True, PATCH),           # ... reflect, 16 x 16
    "P6": ("fwd", 1, 32, 32, 128, 64, 32, 3, 1, 1, False, PATCH),         # <32, 3, true>; concat 128 + 64; four tiles down the image
    "P7": ("fwd", 1, 16, 64, 96, 0, 64, 3, 1, 1, False, PATCH),           # 32-channel chunks, chunk stages <64, 0, true, 32>
    "P7t": ("fwd", 1, 16, 64, 96, 0, 64, 3, 1, 1, False, PATCH + (("conv3x3_patch_chunk_stage", 0),)),    # ... the tap ring <64, 3, true, 32>
    "P8": ("fwd", 2, 16, 64, 32, 64, 32, 3, 1, 1, True, PATCH),           # <32, 0, true, 32>; concat on a 32-channel boundary; reflect
    "P8t": ("fwd", 2, 16, 64, 32, 64, 32, 3, 1, 1, True, PATCH + (("conv3x3_patch_chunk_stage", 0),)),    # <32, 3, true, 32>
    "P9": ("fwd", 1, 16, 64, 32, 0, 256, 3, 1, 1, True, PATCH),           # <128, 0, true, 32>: one 32-channel chunk, two Cout chunks
    "P9t": ("fwd", 1, 16, 64, 32, 0, 256, 3, 1, 1, True, PATCH + (("conv3x3_patch_chunk_stage", 0),)),    # <128, 3, true, 32>
    "P10": ("fwd", 1, 32, 48, 96, 0, 128, 3, 1, 1, True, PATCH),          # <128, 3, true, 32> by default: three 32-channel chunks; 16 x 16
    "T1": ("fwd", 2, 32, 64, 64, 0, 64, 3, 1, 1, False, TALL),            # <64, 0, true, 32, 512>; 16 x 32 tiles
    "T2": ("fwd", 1, 64, 48, 32, 64, 32, 3, 1, 1, True, TALL),            # <32, 0, true, 32, 512>; 32 x 16 tiles, 2 x 3; concat 32 + 64
    "T3": ("fwd", 2, 64, 32, 64, 0, 64, 3, 1, 1, True, TALL),             # <64, .., 512>; 16 x 32 tiles, reflect, four tiles down an image
    "T4": ("fwd", 2, 32, 16, 32, 0, 32, 3, 1, 1, False, TALL),            # <32, .., 512>; 32 x 16, zero padding, n = 2
    # B3. the patch kernel's data-gradient form for a concat layer 64 + 64 -> 256: launched 256 -> 128, all c1 + c2 channels at once
    "G1": ("dgrad", 2, 16, 64, 64, 64, 256, 3, 1, 1, False, PATCH),
    # C. 128-row LDS-DMA tiles with taps, default options (the patch kernel refuses these shapes).  M = 198, 144, 144: ragged
    "C1a": ("fwd", 2, 9, 11, 64, 0, 128, 3, 1, 1, False, ()),              # nine K stages: <128, 128, 4, 2>
    "C1b": ("fwd", 2, 9, 11, 128, 0, 64, 3, 1, 1, True, ()),               # <128, 64, 4, 3>, 18 stages, reflect
    "C1c": ("fwd", 2, 9, 11, 64, 64, 32, 3, 1, 1, False, ()),              # <128, 32, 4, 3>; concat on a 64-channel boundary
    "C2a": ("fwd", 2, 17, 15, 64, 0, 64, 3, 2, 1, True, ()),               # stride 2 on odd sizes -> 9 x 8; reflect
    "C2b": ("fwd", 2, 17, 15, 128, 0, 256, 3, 2, 1, False, ()),            # ... zero padding; two Cout chunks: the XCD-pair grid
    "C3a": ("fwd", 2, 17, 15, 128, 0, 192, 1, 2, 0, False, ()),            # 1x1 stride 2, two K stages: <128, 128, 4, 1, 4>; the second chunk half filled
    "C3b": ("fwd", 2, 17, 15, 64, 0, 128, 1, 2, 0, False, ()),             # one K stage: <128, 128, 4, 2, 4>
    # D1 / D2. vqseg_conv2d_dgrad_s2_f(precise = 0); the id read back is the last parity class's (1 x 1 taps)
    "S2": ("dgrad", 2, 17, 15, 64, 0, 64, 3, 2, 1, True, ()),              # C2a's gradient: odd sizes, padded grid 19 x 17; gy 64: <128, 64, 4, 3>; C4: dilated
    "S3": ("dgrad", 2, 12, 10, 128, 0, 64, 3, 2, 1, False, ()),            # even sizes, padded grid 14 x 12, last row and column 0; <128, 128, 4, 2, 4>
    "S4": ("dgrad", 2, 13, 11, 72, 0, 40, 3, 2, 1, True, ()),              # gy 40 channels: conv_igemm_kernel<64, false, 32>
    "S5": ("dgrad", 2, 12, 10, 24, 0, 40, 3, 2, 1, False, ()),             # ... <32, false, 32>, even sizes
    "S1": ("dgrad", 2, 17, 15, 128, 0, 64, 1, 2, 0, False, ()),            # k = 1 on odd sizes: 9 x 8 gradient pixels onto 17 x 15
    "S1g": ("dgrad", 2, 17, 15, 136, 0, 40, 1, 2, 0, False, ()),           # ... conv_igemm_kernel<128, false, 32>, second chunk 8 channels
    # D3. vqseg_conv2d_dgrad_s2_fold_f: n, h, w, gx channels (c1), gy channels (cout)
    "R1": ("fold", 2, 8, 12, 128, 0, 128, 3, 2, 1, True, ()),              # CLS <128, 128, 4, 1, 4>: 4 * (128 / 64) = 8 stages
    "R2": ("fold", 1, 12, 8, 128, 0, 256, 3, 2, 1, False, ()),             # CLS <128, 128, 4, 2>: deeper K; zero padding
    "R3": ("fold", 2, 20, 20, 72, 0, 64, 3, 2, 1, True, ()),               # CLS <128, 64, 4, 3>; the second chunk has 8 channels
    "R4": ("fold", 3, 4, 36, 256, 0, 128, 3, 2, 1, True, ()),              # the minimum height; two chunks
}

# instantiation id -> the cases whose launch must read it back (launch_conv3x3_patch, launch_conv_impl, launch_dgrad_s2_fold)
VARIANTS = {
    patch_id(128, 3, True, 64): ["P1", "P3", "P3r", "G1"],
    patch_id(256, 2, False, 64): ["P2", "P2z"],
    patch_id(128, 4, True, 64): ["P1u2"],
    patch_id(128, 3, False, 64): ["P1u0"],
    patch_id(64, 3, True, 64): ["P5", "P5r"],
    patch_id(32, 3, True, 64): ["P6"],
    patch_id(64, 0, True, 32): ["P7"],
    patch_id(32, 0, True, 32): ["P8"],
    patch_id(128, 0, True, 32): ["P9"],
    patch_id(64, 3, True, 32): ["P7t"],
    patch_id(32, 3, True, 32): ["P8t"],
    patch_id(128, 3, True, 32): ["P9t", "P10"],
    patch_id(64, 0, True, 32, 512): ["T1", "T3"],
    patch_id(32, 0, True, 32, 512): ["T2", "T4"],
    glds_id(128, 2): ["C1a"],
    glds_id(64, 3): ["C1b", "C2a", "S2"],
    glds_id(32, 3): ["C1c"],
    glds_id(128, 2, pair=True): ["C2b"],
    glds_id(128, 1, 4, pair=True): ["C3a"],
    glds_id(128, 2, 4): ["C3b", "S3", "S1"],
    igemm_id(64): ["S4"],
    igemm_id(32): ["S5"],
    igemm_id(128): ["S1g"],
    glds_id(128, 1, 4, cls=True): ["R1", "R4"],
    glds_id(128, 2, 1, cls=True): ["R2"],
    glds_id(64, 3, 1, cls=True): ["R3"],
}

# what the issue lists for A and D3, in the ids' own digits
A_IDS = (0x3143210, 0x3182200, 0x3144210, 0x3143200, 0x3123210, 0x3113210, 0x3120110, 0x3110110, 0x3140110, 0x3123110, 0x3113110,
         0x3143110, 0x3220110, 0x3210110)
CLS_IDS = (0x1144142, 0x1144212, 0x1124312)

# which test family launches a case (tests/test_fast_conv_gpu.py parametrises over these)
A_CASES = [c for c in CASES if c[0] in "PT"]
EPILOGUE_CASES = ["P3", "P2z", "P5", "P7", "T1"]              # B1 / B2: zero padding, one source (vqseg_conv2d_affine_bits_f takes no other)
C_CASES = [c for c in CASES if c[0] == "C"]
S2_K3_CASES = ["S2", "S3", "S4", "S5"]
S2_K1_CASES = ["S1", "S1g"]
FOLD_CASES = [c for c in CASES if c[0] == "R"]


def variant_of(case):
    (vid,) = [v for v, cs in VARIANTS.items() if case in cs]
    return vid


def geometry(case):
    """the eleven geometry fields of a named case; a tuple (tests/layer_cases.py's census rows) is its own geometry"""
    return tuple(case[:11]) if isinstance(case, tuple) else CASES[case][:11]


def options(case):
    return {} if isinstance(case, tuple) else dict(CASES[case][11])


def kind(case):
    return geometry(case)[0]


def out_size(case):
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def grad_grid(case):
    """(rows, columns, padding of the launched convolution) of a gradient case's output grid, as precise_cases.grad_grid; "fold"
    cases: the PADDED grid their four parity classes live on"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    padded = reflect or stride == 2
    return (h + 2 * pad, w + 2 * pad, k - 1) if padded else (h, w, k - 1 - pad)


def _seed(geom):
    return 20000 + zlib.crc32(repr(geom).encode()) % 50000


@functools.lru_cache(maxsize=None)
def _operands(geom):
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geom
    cin = c1 + c2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    s = _seed(geom)
    act = (n, h, w, cin) if knd == "fwd" else (n, ho, wo, cout)
    wt = (synth.uniform(s + 1, (cout, cin, k, k), -1, 1) * (2.0 / (cin * k * k)) ** 0.5).bfloat16().float()
    return synth.uniform(s, act, -1, 1).bfloat16().float(), wt


def operands(case):
    """fwd: (x [n, h, w, cin], w [cout, cin, k, k]); dgrad / fold: (gy [n, ho, wo, cout], w).  fp32 holding bf16 values; the weights
    scaled (2 / (cin k k)) ** 0.5 as dispatch_cases.operands"""
    return _operands(geometry(case))


def _gemm(geom):
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geom
    a, wt = _operands(geom)
    if knd == "fwd":
        xp = a.permute(0, 3, 1, 2)
        if pad:
            xp = F.pad(xp, (pad,) * 4, mode="reflect" if reflect else "constant")
        return pc._unfold_rows(xp, k, stride), wt.permute(2, 3, 1, 0).reshape(-1, cout).contiguous()
    g = a.permute(0, 3, 1, 2)
    if stride == 2:
        d = torch.zeros(n, cout, 2 * g.shape[2] - 1, 2 * g.shape[3] - 1, dtype=a.dtype)
        d[:, :, ::2, ::2] = g
        g = d
    padded = reflect or stride == 2
    gh, gw, gpad = (h + 2 * pad, w + 2 * pad, k - 1) if padded else (h, w, k - 1 - pad)
    g = F.pad(g, (gpad, gw + k - 1 - gpad - g.shape[3], gpad, gh + k - 1 - gpad - g.shape[2]))
    return pc._unfold_rows(g, k, 1), wt.flip(2, 3).permute(2, 3, 0, 1).reshape(-1, c1 + c2).contiguous()


def gemm(case):
    """(A [rows, K], B [K, columns]) in fp32; gradients: A is the zero-dilated, zero-padded gy's im2col matrix on grad_grid, B the
    tap-flipped transposed image"""
    return _gemm(geometry(case))


@functools.lru_cache(maxsize=None)
def _reference(geom):
    a, b = _gemm(geom)
    a, b = a.double(), b.double()
    return a @ b, a.abs() @ b.abs()


def reference(case):
    """(ref, S) in fp64: A B and |A| |B| ("fold" cases: on the padded grid, before the fold / crop)"""
    return _reference(geometry(case))


def contraction(case):
    """K of the bound: an int, or for a 3x3 stride-2 data gradient a [rows, 1] tensor (taps of the pixel's parity class x channels)"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    if knd == "fwd":
        return k * k * (c1 + c2)
    if stride == 2 and k == 3:
        gh, gw, _gpad = grad_grid(case)
        ti = torch.where(torch.arange(gh) % 2 == 0, 2, 1)
        tj = torch.where(torch.arange(gw) % 2 == 0, 2, 1)
        return (ti[:, None] * tj[None, :] * cout).repeat(n, 1, 1).reshape(-1, 1).double()
    return k * k * cout


def limit(case):
    """dispatch_cases.bound on the case's GEMM, [rows, columns]"""
    ref, S = reference(case)
    return dc.bound(ref, S, contraction(case)).expand_as(ref)


@functools.lru_cache(maxsize=None)
def _autograd_gradient(geom):
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geom
    gy, wt = _operands(geom)
    x = torch.zeros(n, c1 + c2, h, w, dtype=torch.float64, requires_grad=True)
    xp = F.pad(x, (pad,) * 4, mode="reflect" if reflect else "constant") if pad else x
    (g,) = torch.autograd.grad(F.conv2d(xp, wt.double(), stride=stride), x, gy.double().permute(0, 3, 1, 2))
    return g.permute(0, 2, 3, 1).reshape(-1, c1 + c2)


def autograd_gradient(case):
    """the fp64 autograd gradient with respect to the layer's UNPADDED input, through the reflect or zero padding: [n h w, cin]"""
    return _autograd_gradient(geometry(case))


def touched(case):
    """bool [h, w]: the pixels of a reflect "fold" case where reflect_s2_ring_add_kernel adds ring values (x row 1 and column 1)"""
    _kind, n, h, w, *_rest = geometry(case)
    t = torch.zeros(h, w, dtype=torch.bool)
    t[1, :] = True
    t[:, 1] = True
    return t


def fold_parts(case, v):
    """v [n (h + 2) (w + 2), c] on the padded grid -> (body [n, h, w, c], ring [n, h, w, c], terms [h, w]): what the merged kernel
    writes to x itself, the sum of what reflect_s2_ring_add_kernel adds to it (padded row 0 onto x row 1, padded column 0 onto x
    column 1, the corner onto x (1, 1); padded row h + 1 / column w + 1 carry no gradient: h, w even) and the number of padded
    positions per pixel (1, 2, or 4 at (1, 1))"""
    _kind, n, h, w, c1, *_rest = geometry(case)
    g = v.reshape(n, h + 2, w + 2, -1)
    ring = torch.zeros_like(g[:, 1:h + 1, 1:w + 1])
    ring[:, 1, :] += g[:, 0, 1:w + 1]
    ring[:, :, 1] += g[:, 1:h + 1, 0]
    ring[:, 1, 1] += g[:, 0, 0]
    t = torch.ones(h, w)
    t[1, :] += 1
    t[:, 1] += 1
    t[1, 1] += 1
    return g[:, 1:h + 1, 1:w + 1], ring, t


@functools.lru_cache(maxsize=None)
def fold_reference(case):
    """(want, limit) [n h w, c] of a "fold" case; want is the fp64 autograd gradient through the padding.

    Zero padding: the crop of the padded grid's reference and of its bound.  Reflect padding, from reflect_s2_ring_add_kernel's
    comments: the merged kernel rounds every padded position's accumulator to bf16 -- the body into x, padded row 0 / column 0 / the
    corner into the ring --, then the ring kernel unpacks them, sums in fp32 (x (1, 1): ring + ring + ring, then x + that: three
    additions; elsewhere on row 1 / column 1: one) and rounds once.  With b_p = 2^-8 |ref_p| + K_p 2^-23 S_p the bound of
    position p (dispatch_cases.bound: accumulation and that position's rounding), a pixel that sums t positions is within

        E + 2^-8 (|sum_p ref_p| + E),    E = sum_p b_p + (t - 1) 2^-23 sum_p (|ref_p| + b_p)

    E: the parts' own errors and t - 1 fp32 additions of terms of at most |ref_p| + b_p each (one ulp per addition, which also
    covers the partial sums' growth); then the rounding of the computed sum s to bf16, within 2^-8 |s| (half an ulp of 8 significant
    bits, just above a power of two), |s| <= |sum_p ref_p| + E.  A pixel with t = 1 is not touched by the ring kernel and keeps b_p
    alone.  No term comes from a kernel's output."""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    assert knd == "fold"
    ref, S = reference(case)
    b = limit(case)
    want = autograd_gradient(case)
    if not reflect:
        crop = lambda v: v.reshape(n, h + 2, w + 2, c1)[:, 1:-1, 1:-1].reshape(-1, c1)
        assert bool(((want - crop(ref)).abs() <= 1e-13 * crop(S)).all())
        return want, crop(b)
    body, ring, t = fold_parts(case, ref)
    body_b, ring_b, _t = fold_parts(case, b)
    body_a, ring_a, _t = fold_parts(case, ref.abs() + b)
    body_s, ring_s, _t = fold_parts(case, S)
    folded = body + ring
    assert bool(((want.reshape(folded.shape) - folded).abs() <= 1e-13 * (body_s + ring_s)).all())
    # (the general fold also maps padded row h + 1 / column w + 1 onto x row h - 2 / column w - 2: they carry no gradient)
    assert bool(((stem_cases.reflect_fold(ref.reshape(n, h + 2, w + 2, c1)) - folded).abs() <= 1e-13 * (body_s + ring_s)).all())
    t = t[None, :, :, None]
    e = body_b + ring_b + (t - 1) * U * (body_a + ring_a)
    lim = torch.where(t > 1, e + 2.0 ** -8 * (folded.abs() + e), body_b)
    return want, lim.reshape(-1, c1)


@functools.lru_cache(maxsize=None)
def epilogue_operands(case):
    """(scale [c], shift [c], addend [rows, c] holding bf16 values, keep [rows, c] bool) of the fused affine epilogues: scales of both
    signs in 0.5 .. 1.5, shifts in -0.5 .. 0.5"""
    rows, c = reference(case)[0].shape
    s = _seed(geometry(case)) + 100
    scale = synth.uniform(s, (c,), 0.5, 1.5) * torch.where(synth.uniform(s + 1, (c,)) < 0.3, -1.0, 1.0)
    return scale, synth.uniform(s + 2, (c,), -0.5, 0.5), synth.uniform(s + 3, (rows, c), -1, 1).bfloat16().float(), synth.uniform(s + 4, (rows, c)) < 0.5


def pack_bits(keep):
    """bool [rows, c] -> uint8 [rows c / 8]: element e of the flattened tensor is bit e % 8 of byte e / 8"""
    return (keep.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def epilogue_reference(case, form):
    """(y_ref, limit) in fp64 of form "affine" (y = relu(t + addend)) or "bits" (y = t + (keep ? addend : 0)), t = acc scale + shift.
    The kernel rounds t to bf16, adds the bf16 addend in fp32 and rounds again:  |y - y_ref| <= 2^-8 |y_ref| + 2^-8 |t_ref| +
    K 2^-23 S |scale|, as test_dispatch_variants_gpu derives it (each rounding within 2^-9 of its argument, which differs from the
    fp64 one by terms already counted; ReLU does not increase a difference)."""
    ref, S = reference(case)
    scale, shift, res, keep = epilogue_operands(case)
    t_ref = ref * scale.double() + shift.double()
    y_ref = torch.relu(t_ref + res.double()) if form == "affine" else t_ref + torch.where(keep, res.double(), torch.zeros((), dtype=torch.float64))
    return y_ref, 2.0 ** -8 * y_ref.abs() + 2.0 ** -8 * t_ref.abs() + contraction(case) * U * S * scale.double().abs()


# ---------------------------------------------------------------------------------------------------------------------------
# the documented arithmetic on the CPU, and the ways it goes wrong
# ---------------------------------------------------------------------------------------------------------------------------
def round_bf16(v):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    return v.bfloat16().float()


def truncate_bf16(v):
    """fp32 -> bf16 by dropping the low 16 bits"""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


TILE_W = 32                                                 # the 8 x 32 pixel tile of the emulated patch case ("halo")


def chunk_width(case):
    """channels per K chunk: 64 where every tap's channel range is whole 64-channel chunks (launch_conv_impl's k64), else 32"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    c = c1 + c2 if knd == "fwd" else cout
    split = c1 if knd == "fwd" and c2 else c
    return 64 if c % 64 == 0 and split % 64 == 0 else 32


def emulate(case, mutation=None):
    """The kernels' arithmetic on the CPU: products of bf16 values are exact in fp32, summed in fp32 (one fp32 matmul), the
    accumulator rounded to the nearest bf16; "fold" cases then take the padded grid's rounded values through emulate_fold.
    Mutations, each a way a tiled bf16 kernel goes wrong:
      truncate  the store drops the accumulator's low 16 bits instead of rounding to nearest
      chunk     one 64- / 32-channel chunk of one tap (the middle tap's last chunk) is left out of the contraction
      halo      (forward 3x3, W a multiple of 2 TILE_W) the left neighbour of the pixels in column TILE_W -- the halo column of the
                second tile -- reads as zero for the tap (kh, kw) = (1, 0)
      row       the last output row (fold: of the unpadded gradient) is replaced by the nearest one above it whose reference differs
                (a clamped ragged tail)
      corner    (reflect fold) x (1, 1) misses the padded corner's contribution"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    a, b = gemm(case)
    c = a.shape[1] // (k * k)
    if mutation == "chunk":
        ck = chunk_width(case)
        q0 = (k * k // 2) * c + (c - 1) // ck * ck
        a = a.clone()
        a[:, q0:(k * k // 2) * c + c] = 0
    elif mutation == "halo":
        assert knd == "fwd" and k == 3 and stride == 1 and w % (2 * TILE_W) == 0
        edge = (torch.arange(w) == TILE_W).repeat(n * h)
        a = a.clone()
        a[edge, 3 * c:4 * c] = 0
    acc = a @ b
    y = truncate_bf16(acc) if mutation == "truncate" else round_bf16(acc)
    ref = reference(case)[0]
    if knd == "fold":
        y = emulate_fold(case, y, mutation)
        ref = fold_reference(case)[0]
    if mutation == "row":
        y[-1] = y[int((ref[:-1] != ref[-1]).any(1).nonzero().max())]
    return y


def emulate_fold(case, parts, mutation=None):
    """parts [n (h + 2) (w + 2), c], bf16 values on the padded grid -> [n h w, c]: the crop (zero padding) or the ring kernel's sum,
    x + (ring [+ ring + ring]) in fp32 in reflect_s2_ring_add_kernel's order, rounded once"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = geometry(case)
    g = parts.reshape(n, h + 2, w + 2, c1)
    x = g[:, 1:h + 1, 1:w + 1].clone()
    if reflect:
        v = torch.zeros_like(x)
        v[:, 1, :] = g[:, 0, 1:w + 1]                       # padded row 0, columns 1 .. w -> x (1, 0 .. w - 1)
        v[:, :, 1] = torch.where(torch.arange(h)[None, :, None] == 1, v[:, :, 1] + g[:, 1:h + 1, 0], g[:, 1:h + 1, 0])
        if mutation != "corner":
            v[:, 1, 1] = v[:, 1, 1] + g[:, 0, 0]
        t = touched(case)
        x[:, t] = round_bf16(x[:, t] + v[:, t])
    return x.reshape(-1, c1)
