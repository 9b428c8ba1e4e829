"""Shapes, operands, fp64 references, the acceptance bound and a CPU emulation of the fp32 ("precise", split-bf16) convolution
kernels: conv_igemm_kernel<128 | 64 | 32, true, 32> (forward, data gradients, fused epilogues) and conv_wgrad_kernel<TM, TN, true>
(per-tap weight gradient), plus bf16-exact operands for their fast-mode siblings <.., false, 32> / <TM, TN, false>.
tests/test_precise_conv_gpu.py runs the kernels against this; tests/test_precise_bound_cpu.py checks the bound itself without a GPU.

Every case is a GEMM  out[r, j] = sum_q A[r, q] B[q, j]  over the same fp32 values the kernel reads:
    forward / data gradient   A = the im2col matrix of the launched convolution, columns in the kernel's K order (tap, channel),
                              B = the weight image [(tap, channel), output channel]; rows = output pixels
    weight gradient           A = gy^T [Cout, M], B = the im2col matrix of x [M, (tap, ci)]: the contraction runs over the M pixels
The reference is A B in fp64, next to S = |A| |B| (the scale of every error term).  Operands and references are computed once per case
and shared; nobody writes into them.

The bound for fp32 outputs, elementwise, with no term from the code under test:

    |y - ref| <= 2^-16 S + 3 K 2^-23 S + 2^-23 |ref|

  * the kernels split a = hi + lo with hi = bf16(a), lo = bf16(a - hi), both round-to-nearest-even to 8 significant bits; the weights
    are pre-split the same way.  Of a b = (a_hi + a_lo + ra)(b_hi + b_lo + rb) they keep a_lo b_hi + a_hi b_lo + a_hi b_hi (each
    product of two bf16 values is exact in fp32) and leave out a_lo b_lo, ra b and a rb;
  * the split term 2^-16 S is the one the kernels' "~2^-16 relative per product" claims, and it is what an operand pays ON AVERAGE,
    not in the worst case.  Half an ulp of 8 significant bits is 2^-8 of a value just above a power of two: |a_lo| <= 2^-8 |a|,
    |ra| <= 2^-17 |a| (a - hi has its leading bit at least 9 places down, and lo keeps 8 bits of it), so ONE product can be off by
    2^-16 + 2 2^-17 = 2^-15 |a b| -- when both operands sit just above a power of two with both roundings at half an ulp
    (test_precise_bound_cpu asserts 2^-8 and 2^-17 on the operands, and that 2^-18 does not hold).  A mantissa drawn uniformly from
    [1, 2) has E |a_lo| / |a| = ln 2 * 2^-9, so the omitted a_lo b_lo is about 2^-19 |a b| on average, the two residuals less, and
    their signs are independent across the K products of an element, while 2^-16 S grants every product 2^-16 with the same sign.
    So 2^-16 S, HALF the worst case, is a bound for sums of independent full-mantissa operands -- these cases: the documented
    arithmetic emulated on the CPU on the same operands stays below 0.7 of the whole bound on the 8- to 48-term sums of S2 / S3 and
    below 0.25 everywhere else (test_precise_bound_cpu asserts it inside on every element) -- and not for adversarial ones.  It
    is kept at the kernels' own claim rather than doubled: a correct kernel passes on the committed operands either way, and the
    tighter figure is the one the mutations have to violate;
  * 3 K fp32 additions in any order err by at most 3 K u (sum of |terms|), |terms| summing to at most (1 + 2^-8) S; u = 2^-23 (one
    ulp, not half of one) as in tests/dispatch_cases.py covers an adder that truncates and that factor;
  * 2^-23 |ref|: room for the output's own rounding (the accumulator IS the fp32 output: nothing is lost there);
  * K, the contraction length: taps x channels of the convolution actually launched -- per output pixel for the parity classes of a
    stride-2 data gradient (2 x 2, 2 x 1, 1 x 2 or 1 x 1 taps; the dilated launch of the same gradient runs over all nine, but the
    others meet exact zeros and x + 0 rounds nothing, so it is held to the same K); weight gradient: K = M + ceil(M / 32): a slab
    holds at least one 32-pixel stage, so the fixed-order slab sum (in fp64, rounded once) cannot add more roundings than that;
  * accumulate = 1: y = prev + gradient in fp32 adds 2^-23 |prev + ref|.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from tests import synth

U = 2.0 ** -23
STAGE = 32                                                  # channels (weight gradient: pixels) per K stage of the precise kernels
SHARP_K = 128                                               # up to this contraction length the split term dominates the bound

# name -> kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, accumulate.  Geometry is always the FORWARD layer's (x [n, h, w, c1 + c2]
# -> y [n, ho, wo, cout]); kind says which of its three GEMMs the case is:
#   fwd     the forward convolution
#   dgrad   the data gradient with respect to the (reflect or stride 2: padded) input, the GEMM over gy with the transposed, tap-flipped
#           weights; stride 2: over the zero-dilated gy
#   wgrad   the weight gradient
# The smallest shapes that reach each instantiation: launch_conv_impl picks BN by the launched Cout alone (>= 128, >= 64, else 32),
# launch_wgrad_impl TM by Cout (>= 128: 4, >= 64: 2, else 1) and TN by Cin % 128 == 0 (4, else 1).
CASES = {
    # forward.  M = 198, 35, 189, 144, 198, 130: never a multiple of the 128-row tile
    "F1": ("fwd", 2, 9, 11, 12, 20, 20, 3, 1, 1, False, 0),     # BN 32; concat split inside a stage; zero padding; K = 288
    "F2": ("fwd", 1, 13, 10, 20, 0, 72, 3, 2, 1, True, 0),      # BN 64; Cin tail (20 of 32); stride 2 on odd sizes, reflect; K = 180
    "F3": ("fwd", 3, 7, 9, 32, 32, 136, 1, 1, 0, False, 0),     # BN 128, second chunk 8 channels; split on a stage boundary; K = 64
    "F4": ("fwd", 1, 12, 12, 8, 0, 128, 3, 1, 1, True, 0),      # BN 128; Cin tail (8 of 32); reflect; K = 72
    "F5": ("fwd", 2, 9, 11, 12, 20, 20, 1, 1, 0, False, 0),     # BN 32; concat split inside THE stage; K = 32
    "F6": ("fwd", 1, 13, 10, 72, 0, 72, 1, 1, 0, False, 0),     # BN 64; three K stages per tap (32, 32, 8): both register sets; K = 72
    # stride-1 data gradient (launched Cin = the layer's Cout, launched Cout = the layer's Cin)
    "D1": ("dgrad", 2, 9, 11, 72, 0, 8, 3, 1, 1, False, 0),     # zero padding: pad 1 on the input grid; BN 64; K = 72; M = 198
    "D2": ("dgrad", 2, 8, 7, 20, 0, 12, 3, 1, 1, True, 0),      # reflect: full correlation on the 10 x 9 grid, then the fold; BN 32; K = 108; M = 180
    # stride-2 data gradient: parity classes / dilated grid
    "S1": ("dgrad", 2, 17, 15, 136, 0, 32, 1, 2, 0, False, 0),  # k = 1 on odd h, w: 9 x 8 gradient pixels onto the 17 x 15 grid; BN 128; K = 32
    "S2": ("dgrad", 3, 13, 11, 72, 0, 12, 3, 2, 1, True, 0),    # k = 3, odd sizes: padded grid 15 x 13; BN 64; K = 12 .. 48
    "S3": ("dgrad", 3, 12, 10, 20, 0, 8, 3, 2, 1, False, 0),    # k = 3, even sizes: padded grid 14 x 12; BN 32; K = 8 .. 32
    # weight gradient.  M = 70, 126 (ragged last 32-pixel stage), 288 (two slabs of 160 + 128 pixels)
    "W1": ("wgrad", 1, 7, 10, 128, 0, 136, 3, 1, 1, False, 0),  # <4, 4>; 3x3 zero padding
    "W2": ("wgrad", 1, 7, 10, 12, 12, 136, 3, 1, 1, True, 0),   # <4, 1>; reflect; concat split inside the 32-channel tile
    "W3": ("wgrad", 1, 7, 10, 128, 0, 72, 1, 1, 0, False, 0),   # <2, 4>; 1x1
    "W4": ("wgrad", 2, 13, 10, 24, 0, 72, 3, 2, 1, True, 0),    # <2, 1>; 3x3 stride 2 reflect on odd sizes -> 7 x 5
    "W5": ("wgrad", 2, 13, 10, 128, 0, 40, 1, 2, 0, False, 0),  # <1, 4>; 1x1 stride 2
    "W6": ("wgrad", 1, 7, 10, 24, 0, 40, 3, 1, 1, False, 1),    # <1, 1>; accumulate
    "W7": ("wgrad", 2, 7, 9, 8, 16, 40, 3, 1, 1, False, 1),     # <1, 1>; M = 126; concat; accumulate
    "W8": ("wgrad", 2, 12, 12, 24, 0, 72, 3, 1, 1, False, 0),   # <2, 1>; M = 288: two slabs; also launched as two uses of one image each
    "W9": ("wgrad", 2, 12, 12, 128, 0, 136, 1, 1, 0, False, 0), # <4, 4>; M = 288: two slabs
    # fast mode (bf16-exact operands, no split): conv_igemm_kernel<.., false, 32> needs Cin % 64 != 0 (or a concat split off 64)
    "G1": ("fwd", 2, 9, 11, 24, 0, 136, 1, 1, 0, False, 0),     # BN 128
    "G2": ("fwd", 1, 13, 10, 40, 0, 72, 3, 2, 1, True, 0),      # BN 64; stride 2 reflect
    "G3": ("fwd", 2, 9, 11, 40, 56, 24, 1, 1, 0, False, 0),     # BN 32; Cin = 96, concat
    # ... conv_wgrad_kernel<TM, TN, false>: shapes the nine-tap and 1x1 plans refuse (Cout % 32 != 0, Wo % 16 != 0, Cin % 32 != 0)
    "V1": ("wgrad", 1, 7, 10, 128, 0, 136, 3, 1, 1, False, 0),
    "V2": ("wgrad", 1, 7, 10, 8, 16, 136, 3, 1, 1, True, 0),
    "V3": ("wgrad", 1, 7, 10, 128, 0, 72, 1, 1, 0, False, 0),
    "V4": ("wgrad", 2, 13, 10, 24, 0, 72, 3, 2, 1, True, 0),
    "V5": ("wgrad", 2, 13, 10, 128, 0, 40, 1, 2, 0, False, 0),
    "V6": ("wgrad", 2, 12, 12, 24, 0, 40, 3, 1, 1, False, 0),   # M = 288: two slabs
}
PRECISE = [c for c in CASES if c[0] in "FDSW"]
FAST = [c for c in CASES if c[0] in "GV"]

# instantiation id (conv_internal.h: conv_variant_igemm(bn, precise, 32, false) = 0x20B01P0, conv_variant_wgrad_tap(tm, tn, precise) =
# 0x60MN0P0) -> the cases that reach it
VARIANTS = {
    0x2040110: ["F3", "F4", "S1"], 0x2020110: ["F2", "F6", "D1", "S2"], 0x2010110: ["F1", "F5", "D2", "S3"],
    0x6044010: ["W1", "W9"], 0x6041010: ["W2"], 0x6024010: ["W3"], 0x6021010: ["W4", "W8"], 0x6014010: ["W5"], 0x6011010: ["W6", "W7"],
    0x2040100: ["G1"], 0x2020100: ["G2"], 0x2010100: ["G3"],
    0x6044000: ["V1"], 0x6041000: ["V2"], 0x6024000: ["V3"], 0x6021000: ["V4"], 0x6014000: ["V5"], 0x6011000: ["V6"],
}


def _row(case):
    """the twelve fields of a named case; a tuple (tests/layer_cases.py's census rows) is its own row"""
    return case if isinstance(case, tuple) else CASES[case]


def variant_of(case):
    (vid,) = [v for v, cs in VARIANTS.items() if case in cs]
    return vid


def kind(case):
    return _row(case)[0]


def fast(case):
    return not isinstance(case, tuple) and case[0] in "GV"


def out_size(case):
    """(ho, wo) of the forward layer"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def grad_grid(case):
    """(rows, columns, padding of the launched convolution) of a data-gradient case's output grid: the input grid of a stride-1
    zero-padded layer, else the PADDED input grid (reflect: folded afterwards; stride 2 with zero padding: cropped)"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    padded = reflect or stride == 2
    return (h + 2 * pad, w + 2 * pad, k - 1) if padded else (h, w, k - 1 - pad)


def _seed(case):
    if isinstance(case, tuple):
        return 40000 + zlib.crc32(repr(case).encode()) % 50000
    return 7000 + 31 * sorted(CASES).index(case)


def full_mantissa(seed, shape):
    """fp32 values sign * m * 2^e with a full random mantissa m in [1, 2); three quarters of the exponents in {-1, 0, 1}, the rest
    uniform in -20 .. -2, so magnitudes span [2^-20, 4] and no lo part underflows; about 3 % exact zeros and 10 % bf16-exact values"""
    m = 1.0 + synth.uniform(seed, shape)
    ue = synth.uniform(seed + 1, shape)
    e = torch.where(ue < 0.75, torch.floor(ue * 4) - 1, -2 - torch.floor((ue - 0.75) * 4 * 19)).to(torch.int32)
    v = torch.ldexp(m, e) * torch.where(synth.uniform(seed + 2, shape) < 0.5, -1.0, 1.0)
    us = synth.uniform(seed + 3, shape)
    v = torch.where((us >= 0.03) & (us < 0.13), v.bfloat16().float(), v)
    return torch.where(us < 0.03, torch.zeros(()), v)


@functools.lru_cache(maxsize=None)
def operands(case):
    """fwd: (x [n, h, w, cin], w [cout, cin, k, k]); dgrad: (gy [n, ho, wo, cout], w); wgrad: (x, gy, prev [cout, cin, k, k] or None).
    fp32; the fast cases hold bf16 values only."""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    cin = c1 + c2
    ho, wo = out_size(case)
    s = _seed(case)
    if fast(case):
        gen = lambda sd, shape: synth.uniform(sd, shape, -1, 1).bfloat16().float()
    else:
        gen = full_mantissa
    if knd == "fwd":
        return gen(s, (n, h, w, cin)), gen(s + 10, (cout, cin, k, k))
    if knd == "dgrad":
        return gen(s, (n, ho, wo, cout)), gen(s + 10, (cout, cin, k, k))
    return gen(s, (n, h, w, cin)), gen(s + 10, (n, ho, wo, cout)), (gen(s + 20, (cout, cin, k, k)) if acc else None)


def _unfold_rows(xp, k, stride):
    """[n, c, H, W] -> [pixels, taps * c], columns (tap, channel): the kernels' K order"""
    n, c = xp.shape[:2]
    cols = F.unfold(xp, k, stride=stride)                   # [n, c * taps, L], rows (channel, tap)
    return cols.transpose(1, 2).reshape(-1, c, k * k).transpose(1, 2).reshape(-1, k * k * c)


def patches(case, x):
    """the forward layer's im2col matrix [M, taps * cin] of x [n, h, w, cin] (any float dtype)"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    xp = x.permute(0, 3, 1, 2)
    if pad:
        xp = F.pad(xp, (pad,) * 4, mode="reflect" if reflect else "constant")
    return _unfold_rows(xp, k, stride)


def grad_patches(case, gy):
    """the data-gradient launch's im2col matrix [grid pixels, taps * cout] of gy [n, ho, wo, cout]: zero-dilated for stride 2"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    g = gy.permute(0, 3, 1, 2)
    if stride == 2:
        d = torch.zeros(n, cout, 2 * g.shape[2] - 1, 2 * g.shape[3] - 1, dtype=gy.dtype)
        d[:, :, ::2, ::2] = g
        g = d
    gh, gw, gpad = grad_grid(case)
    g = F.pad(g, (gpad, gw + k - 1 - gpad - g.shape[3], gpad, gh + k - 1 - gpad - g.shape[2]))
    return _unfold_rows(g, k, 1)


def gemm(case):
    """(A [rows, K], B [K, columns]) in the operands' dtype (fp32)"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    ops = operands(case)
    if knd == "fwd":
        return patches(case, ops[0]), ops[1].permute(2, 3, 1, 0).reshape(-1, cout).contiguous()
    if knd == "dgrad":
        return grad_patches(case, ops[0]), ops[1].flip(2, 3).permute(2, 3, 0, 1).reshape(-1, c1 + c2).contiguous()
    return ops[1].reshape(-1, cout).t().contiguous(), patches(case, ops[0])


@functools.lru_cache(maxsize=None)
def reference(case):
    """(ref, S) in fp64: A B and |A| |B|.  Weight gradient: [cout, taps * cin] (see to_rows); with accumulate, ref does NOT hold prev"""
    a, b = gemm(case)
    a, b = a.double(), b.double()
    return a @ b, a.abs() @ b.abs()


def to_rows(case, gw):
    """a weight gradient in nn.Conv2d's layout [cout, cin, k, k] -> the reference's [cout, (tap, ci)]"""
    return gw.permute(0, 2, 3, 1).reshape(gw.shape[0], -1)


@functools.lru_cache(maxsize=None)
def autograd_reference(case):
    """the same gradient from autograd in fp64 on the explicitly padded input, in the reference's layout (dgrad, wgrad)"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    cin = c1 + c2
    ops = operands(case)
    if knd == "dgrad":
        gh, gw, _gpad = grad_grid(case)
        padded = reflect or stride == 2
        xp = torch.zeros(n, cin, gh, gw, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(xp, ops[1].double(), stride=stride, padding=0 if padded else pad)
        (g,) = torch.autograd.grad(y, xp, ops[0].double().permute(0, 3, 1, 2))
        return g.permute(0, 2, 3, 1).reshape(-1, cin)
    xp = ops[0].double().permute(0, 3, 1, 2)
    if pad:
        xp = F.pad(xp, (pad,) * 4, mode="reflect" if reflect else "constant")
    return to_rows(case, torch.nn.grad.conv2d_weight(xp, (cout, cin, k, k), ops[1].double().permute(0, 3, 1, 2), stride=stride))


def contraction(case):
    """K of the bound: an int, or for a 3x3 stride-2 data gradient a [rows, 1] tensor (taps of the pixel's parity class x channels)"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    if knd == "wgrad":
        ho, wo = out_size(case)
        m = n * ho * wo
        return m + (m + STAGE - 1) // STAGE
    if knd == "dgrad":
        if stride == 2 and k == 3:
            gh, gw, _gpad = grad_grid(case)
            ti = torch.where(torch.arange(gh) % 2 == 0, 2, 1)
            tj = torch.where(torch.arange(gw) % 2 == 0, 2, 1)
            return (ti[:, None] * tj[None, :] * cout).repeat(n, 1, 1).reshape(-1, 1).double()
        return k * k * cout
    return k * k * (c1 + c2)


def sharp(case):
    K = contraction(case)
    return not fast(case) and (K if isinstance(K, int) else int(K.max())) <= SHARP_K


def bound(ref, S, K, total=None):
    """see the module docstring; total = prev + ref of an accumulating launch"""
    b = 2.0 ** -16 * S + 3 * K * U * S + U * ref.abs()
    return b if total is None else b + U * total.abs()


def violations(y, ref, S, K, prev=None):
    """coordinates of the elements of y outside the bound (NaN counts as outside); prev: what an accumulating launch added to"""
    total = None if prev is None else prev.double() + ref
    want = ref if prev is None else total
    return (~((y.double() - want).abs() <= bound(ref, S, K, total))).nonzero()


def worst(y, ref, S, K, prev=None):
    """largest error / bound over the elements with a non-zero bound (the others must be exact: violations sees them)"""
    total = None if prev is None else prev.double() + ref
    b = bound(ref, S, K, total)
    e = (y.double() - (ref if prev is None else total)).abs()
    return float((e[b > 0] / b[b > 0]).max())


def stages(case):
    """the K stages as (first column, one past the last): per tap 32-channel chunks, the last one short; weight gradient: 32 pixels"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    if knd == "wgrad":
        ho, wo = out_size(case)
        m = n * ho * wo
        return [(q, min(q + STAGE, m)) for q in range(0, m, STAGE)]
    c = cout if knd == "dgrad" else c1 + c2
    return [(t * c + q, t * c + min(q + STAGE, c)) for t in range(k * k) for q in range(0, c, STAGE)]


def second_source(case):
    """bool mask over (tap, channel) columns: the channels of the second concat source; None without a concat"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = _row(case)
    if not c2 or knd == "dgrad":
        return None
    return (torch.arange(c1 + c2) >= c1).repeat(k * k)


def split(v):
    """(hi, lo) as the kernels form them: hi = bf16(v), lo = bf16(v - hi), round to nearest even, returned as fp32"""
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


MUTATIONS = ("m1", "m2", "m3", "m4", "m5")
M5_COLUMN = -3                                              # the output column whose weights m5 shifts


def emulate(case, mutation=None):
    """The arithmetic of the kernel comment on the CPU: both operands split, a_lo b_hi + a_hi b_lo + a_hi b_hi as three fp32 matmuls,
    summed in fp32 (an accumulating case: added to prev in fp32).  Mutations, each a way a tiled split kernel goes wrong:
      m1  the a_lo b_hi product dropped everywhere
      m2  ... on one K stage only (the middle one)
      m3  the lo image of the second concat source dropped (cases with a concat)
      m4  the last output row replaced by its neighbour (a ragged tail clamped instead of masked) -- the nearest row above it whose
          reference differs: the last rows of an even-sized stride-2 gradient's padded grid are both zero
      m5  one output column's B column rolled by one K stage (a weight row fetched at the wrong offset; a single-stage case: by half)"""
    a, b = gemm(case)
    ah, al = split(a)
    bh, bl = split(b)
    if mutation == "m1":
        al = torch.zeros_like(al)
    elif mutation == "m2":
        st = stages(case)
        q0, q1 = st[len(st) // 2]
        al = al.clone()
        al[:, q0:q1] = 0
    elif mutation == "m3":
        sec = second_source(case)
        if kind(case) == "wgrad":
            bl = bl.clone()
            bl[:, sec] = 0
        else:
            al = al.clone()
            al[:, sec] = 0
    elif mutation == "m5":
        shift = STAGE if b.shape[0] > STAGE else b.shape[0] // 2
        bh, bl = bh.clone(), bl.clone()
        bh[:, M5_COLUMN] = torch.roll(bh[:, M5_COLUMN], shift)
        bl[:, M5_COLUMN] = torch.roll(bl[:, M5_COLUMN], shift)
    y = al @ bh + ah @ bl + ah @ bh
    if mutation == "m4":
        ref = reference(case)[0]
        y[-1] = y[int((ref[:-1] != ref[-1]).any(1).nonzero().max())]
    prev = operands(case)[2] if kind(case) == "wgrad" else None
    return y if prev is None else to_rows(case, prev) + y


def prev_rows(case):
    """what an accumulating weight-gradient case adds to, in the reference's layout; None otherwise"""
    prev = operands(case)[2] if kind(case) == "wgrad" else None
    return None if prev is None else to_rows(case, prev)
