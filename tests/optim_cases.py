"""References, builders and assertion functions for the optimiser step and the weight-image kernels (csrc/optim_kernels.hip,
csrc/conv_pack.hip).  Not a test module.  tests/test_optim_parity_gpu.py feeds the assertion functions what the kernels returned,
tests/test_optim_parity_cpu.py feeds them emulations that carry one defect each.  Nothing here touches the GPU at import.

Bars.  None is fitted to a kernel's output; u = 2^-24.
  * p, m, v against `adam_emulate` -- the operation chain of `adam_one` in float32 with both fmas rounded ONCE: bit for bit, NaNs by
    position, signed zeros by bits;
  * every image against the NumPy layouts (`image_fwd`, `image_tr`, `image_s3`, `image_s2`): bit for bit, padding zero;
  * p, m, v against `adam_fp64` (one step in float64 from the same float32 state): per element, counted from the roundings of
    `adam_one` (`fp64_bars`), and asserted to lie below the max-norm bars of tests/test_optim_gpu.py at the tensor's scale;
  * the emulation against torch.optim.Adam on the CPU: moments bit for bit, parameters within TORCH_P_BAR_ULP (twice the measured
    TORCH_P_MEASURED_ULP) in units of max(ulp(p_new), ulp(update)).
Measured figures: profiles/optim_parity.md."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
GUARD = 64                                        # sentinel words before and after every guarded allocation
F32_SENTINEL = 0x7FC5A5A5                         # a NaN with a payload no arithmetic produces
I16_SENTINEL = 0x6B6B
I16_FILL = 0x3FC1                                 # what an image holds before the kernel runs: non-zero, so unwritten padding shows
ADAM_CHUNK = 4096                                 # VQSEG_ADAM_CHUNK
PACK_GRID_CAP = 4096 * 256                        # elements one pass of a grid-stride pack kernel covers

# the bars of tests/test_optim_gpu.py (largest difference / largest magnitude) that the counted bars must stay below
OLD_P_BAR, OLD_MOMENT_BAR = 2.5e-7, 1e-7

# emulation against torch.optim.Adam(foreach=False, fused=False) on the CPU, parameters, in units of max(ulp(p_new), ulp(update)):
# measured by tests/test_optim_parity_cpu.py::test_emulation_against_torch_adam_on_the_cpu (6 steps x 200 000 elements, gradients over
# five decades, state re-synchronised each step), bar = twice that (ATen's vectorised sqrt / div differ between builds and between
# the vector body and the scalar tail)
TORCH_P_MEASURED_ULP = 3.0
TORCH_P_BAR_ULP = 2 * TORCH_P_MEASURED_ULP


def note(family, what, err, bar):
    """every check prints its figure and its bar before it asserts (pytest -s: the source of profiles/optim_parity.md)"""
    print(f"[{family}] {what}: {err:.3e} against {bar:.3e}" + (f" ({err / bar:.3f} of it)" if bar > 0 else ""))


# ---------------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------------
def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(a32):
    """round-to-nearest-even bf16 of finite float32 values, as uint16"""
    u = f32_bits(a32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def ulp32(x):
    """spacing of float32 at |x| (x float64 or float32, finite): 2^(floor(log2 |x|) - 23), 2^-149 below the normal range"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    e = np.where(np.ldexp(1.0, e.astype(np.int64)) > np.maximum(a, 2.0 ** -126), e - 1, e)      # log2 rounding at a power of two
    return np.ldexp(1.0, (e - 23).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------
# the Adam rule: float32 emulation with exact fmas, float64 reference, counted bars
# ---------------------------------------------------------------------------------------------------------------------
def adam_scalars(lr, b1, b2, eps, step):
    """the six float32 scalars of vqseg_adam_step_f32: formed in double, cast once (math.pow / math.sqrt are the host's pow / sqrt)"""
    bc1 = 1.0 - math.pow(b1, float(step))
    bc2 = 1.0 - math.pow(b2, float(step))
    return dict(w1=np.float32(1.0 - b1), b2=np.float32(b2), a2=np.float32(1.0 - b2), bc2_sqrt=np.float32(math.sqrt(bc2)),
                eps=np.float32(eps), neg_step=np.float32(-(lr / bc1)))


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, rounded ONCE.  a b is exact in float64 (48 bits).  x + c in float64 is one rounding and the
    cast to float32 a second: they disagree with a single rounding only where the float64 sum is EXACTLY halfway between two float32
    numbers while the exact sum is not -- TwoSum gives the exact remainder, and such a tie is broken towards it.  (Every float32
    midpoint, subnormal ones included, is a float64 number and rounding is monotonic, so no other case exists.)"""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    with np.errstate(all="ignore"):
        x = a * b
        s = x + c
        bb = s - x
        err = (x - (s - bb)) + (c - bb)                                # exact: s + err == a b + c
        r = s.astype(np.float32)
        r64 = r.astype(np.float64)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & (r64 != s)
        up = s > r64
        other = np.nextafter(r, np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
        fmax = float(np.finfo(np.float32).max)
        inf_tie = np.isinf(r64) & (np.abs(s) == fmax + 2.0 ** 103)    # halfway between the largest float32 and 2^128
        other = np.where(inf_tie, np.sign(s) * fmax, other)
        tie = fix & (inf_tie | (np.abs(s - r64) == np.abs(other - s)))
        hi, lo = np.maximum(r64, other), np.minimum(r64, other)
        r = np.where(tie, np.where(err > 0, hi, lo), r64).astype(np.float32)
    return r


def fma32_fraction(a, b, c):
    """the same for finite scalars through rational arithmetic (the independent check of fma32; ~25 us per element)"""
    return round_fraction_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def round_fraction_f32(q):
    """a Fraction -> the nearest float32, ties to even, one rounding (gradual underflow; overflow to inf)"""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1                                                          # 2^e <= q < 2^(e + 1)
    step = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(q, step)
    n = int(n)
    if rem * 2 > step or (rem * 2 == step and n % 2):
        n += 1
    v = n * step
    return np.float32(sign * (math.inf if v >= Fraction(2) ** 128 else float(v)))


def adam_emulate(p, g, m, v, lr, b1, b2, eps, step, defect=None):
    """`adam_one` of csrc/optim_kernels.hip, operation by operation, in float32 -> (p, m, v) float32.
    defect (tests/test_optim_parity_cpu.py): 'm_unfused', 'v_unfused', 'bc2_inside_sqrt', 'eps_before_div', 'skip_last'."""
    s = adam_scalars(lr, b1, b2, eps, step)
    f = np.float32
    p, g, m, v = (np.array(t, dtype=np.float32) for t in (p, g, m, v))
    with np.errstate(all="ignore"):
        d = (g - m).astype(f)
        m1 = (m + (s["w1"] * d).astype(f)).astype(f) if defect == "m_unfused" else fma32(s["w1"], d, m)
        ag, vb = (s["a2"] * g).astype(f), (v * s["b2"]).astype(f)
        v1 = (vb + (ag * g).astype(f)).astype(f) if defect == "v_unfused" else fma32(ag, g, vb)
        if defect == "bc2_inside_sqrt":
            den = (np.sqrt((v1 / (s["bc2_sqrt"] * s["bc2_sqrt"]).astype(f)).astype(f)).astype(f) + s["eps"]).astype(f)
        elif defect == "eps_before_div":
            den = ((np.sqrt(v1).astype(f) + s["eps"]).astype(f) / s["bc2_sqrt"]).astype(f)
        else:
            den = ((np.sqrt(v1).astype(f) / s["bc2_sqrt"]).astype(f) + s["eps"]).astype(f)
        p1 = (p + ((s["neg_step"] * m1).astype(f) / den).astype(f)).astype(f)
    if defect == "skip_last" and p.size:
        for new, old in ((p1, p), (m1, m), (v1, v)):
            new.reshape(-1)[-1] = old.reshape(-1)[-1]
    return p1, m1, v1


def adam_fp64(p, g, m, v, lr, b1, b2, eps, step):
    """one step of the same rule in float64 from the same float32 state and the same float32 scalars
    -> dict(p, m, v, upd, den, d, vb, ag): the results and the intermediates the bars are counted on"""
    s = {k: float(x) for k, x in adam_scalars(lr, b1, b2, eps, step).items()}
    p, g, m, v = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (p, g, m, v))
    d = g - m
    m1 = m + s["w1"] * d
    ag, vb = s["a2"] * g, v * s["b2"]
    v1 = ag * g + vb
    den = np.sqrt(v1) / s["bc2_sqrt"] + s["eps"]
    upd = s["neg_step"] * m1 / den
    return dict(p=p + upd, m=m1, v=v1, upd=upd, den=den, d=d, vb=vb, ag=ag, g=g, s=s)


TINY = 2.0 ** -149


def fp64_bars(r):
    """Per-element bars on |x32 - x64| counted from the roundings of `adam_one`; h(x) = ulp32(x) / 2 is what one correctly rounded
    float32 operation with exact result x can lose (2^-150 in the subnormal range); u = 2^-24 >= h(x) / |x|.
      m: d = g - m one rounding, the fma one:                      bar_m = h(m') + w1 h(d)
      v: a2 g one rounding (then times |g|), v b2 one, the fma one:  bar_v = h(v') + h(v b2) + |g| h(a2 g)
      p: the update ns m' / (sqrt(v') / bc + eps) passes five relative roundings -- sqrt, div, add on the denominator (all terms
         non-negative, so each is at most u of the denominator), mul and div on the quotient -- and inherits bar_m / |m'| from m' and
         half of bar_v / v' (<= u: the square root halves a relative error) from v'; the final add rounds once:
                                                                 bar_p = h(p') + (5 + 1) u |upd| + |ns| bar_m / den
    Each h() is taken at |x| + the error x inherits, each bar carries a factor 1 + 2^-10 for the second-order terms, and the
    quotient terms a floor of two subnormal steps.  Valid where den is a normal number (the callers pass finite, ordinary data)."""
    s = r["s"]
    h = lambda x: ulp32(x) / 2
    bar_m = (h(np.abs(r["m"]) + s["w1"] * h(r["d"])) + s["w1"] * h(r["d"])) * (1 + 2.0 ** -10)
    in_v = h(r["vb"]) + np.abs(r["g"]) * h(r["ag"])
    bar_v = (h(np.abs(r["v"]) + in_v) + in_v) * (1 + 2.0 ** -10)
    in_p = 6 * U * np.abs(r["upd"]) + abs(s["neg_step"]) * bar_m / r["den"] + 2 * TINY
    bar_p = (h(np.abs(r["p"]) + in_p) + in_p) * (1 + 2.0 ** -10)
    return dict(p=bar_p, m=bar_m, v=bar_v)


def adam_data(seed, n, zeros=True):
    """ordinary training-like state: p in (-0.2, 0.2); g over five decades (|g| up to 10), one element in 16 exactly zero;
    m and v of the size a history of such gradients leaves"""
    rs = np.random.RandomState(seed)
    dec = (10.0 ** rs.randint(-3, 2, size=n)).astype(np.float32)
    p = rs.uniform(-0.2, 0.2, size=n).astype(np.float32)
    g = (rs.uniform(-1, 1, size=n).astype(np.float32) * dec).astype(np.float32)
    if zeros and n >= 16:
        g[rs.permutation(n)[:n // 16]] = 0.0
    m = (rs.uniform(-0.5, 0.5, size=n).astype(np.float32) * dec).astype(np.float32)
    v = (rs.uniform(0.05, 1.0, size=n).astype(np.float32) * dec * dec).astype(np.float32)
    return p, g, m, v


def special_values():
    """(p, g, m, v) of about 4k elements: every listed special gradient / state crossed with ordinary partners, then ordinary filler.
    g: +-0, subnormal, g^2 underflowing, g^2 overflowing to inf, +-inf, NaN; v: 0 (with eps = 0: 0 / 0 and x / 0), subnormal;
    m: subnormal, +-0; p: +-0."""
    f = np.float32
    sub = [f(1e-45), f(-1e-45), f(3e-42), f(1.1754942e-38), f(-7e-40)]
    gs = [f(0.0), f(-0.0)] + sub + [f(1e-23), f(-3e-25), f(2e-19), f(3e19), f(-1e21), f(3.3e38), f(np.inf), f(-np.inf), f(np.nan),
                                     f(0.5), f(-1e-3)]
    ms = [f(0.0), f(-0.0), f(1e-45), f(-5e-41), f(1e-39), f(0.25), f(-1e-4)]
    vs = [f(0.0), f(1e-45), f(4e-42), f(1e-38), f(1e-30), f(0.04), f(3e38)]
    ps = [f(0.0), f(-0.0), f(0.1), f(-1e-30)]
    grid = np.array([(p, g, m, v) for g in gs for m in ms for v in vs for p in ps], dtype=np.float32)      # 18 * 7 * 7 * 4 = 3528
    fill = np.stack(adam_data(77, 4100 - grid.shape[0]), axis=1)
    allv = np.concatenate([grid, fill], axis=0)
    allv = allv[np.random.RandomState(78).permutation(allv.shape[0])]                 # specials in every lane and vector slot
    return tuple(np.ascontiguousarray(allv[:, i]) for i in range(4))


def check_bits(got, want, label):
    """float32 arrays equal bit for bit; where `want` is NaN `got` must be NaN (payloads are not compared)"""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, f"{label}: {got.shape} against {want.shape}"
    wn, gn = np.isnan(want), np.isnan(got)
    assert (wn == gn).all(), f"{label}: NaN positions differ at flat indices {np.flatnonzero(wn != gn)[:8]}"
    bad = (f32_bits(got) != f32_bits(want)) & ~wn
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{label}: {i.size} of {got.size} elements differ from the expected bits; first at {i[0]} (got {got[i[0]]!r}, "
                             f"expected {want[i[0]]!r}), last at {i[-1]}")


def check_adam_emulation(got, state, hyper, label, defect=None):
    """got = (p, m, v) after one step from state = (p, g, m, v) with hyper = (lr, b1, b2, eps, step): bit-equal to adam_emulate"""
    want = adam_emulate(*state, *hyper, defect=defect) if defect else adam_emulate(*state, *hyper)
    for i, name in ((1, "m"), (2, "v"), (0, "p")):                     # the moments first: a parameter inherits their defects
        check_bits(got[i], want[i], f"{label} {name} against the float32 emulation")
    return want


def check_adam_fp64(got, state, hyper, label):
    """the counted per-element bars against float64, and the bars themselves against the max-norm bars of tests/test_optim_gpu.py.
    -> {name: worst share of its bar}"""
    r = adam_fp64(*state, *hyper)
    bars = fp64_bars(r)
    worst = {}
    for name, a, old in zip(("p", "m", "v"), got, (OLD_P_BAR, OLD_MOMENT_BAR, OLD_MOMENT_BAR)):
        ref, bar = r[name].reshape(-1), bars[name].reshape(-1)
        assert np.isfinite(ref).all() and np.isfinite(bar).all(), f"{label}: the float64 bound needs finite data"
        scale = float(np.abs(ref).max())
        note("adam fp64", f"{label} {name}: largest counted bar against the old max-norm bar at scale {scale:.3g}", float(bar.max()), old * scale)
        assert bar.max() < old * scale, f"{label}: the counted bar of {name} ({bar.max():.3e}) is not below {old} of the scale {scale:.3e}"
        err = np.abs(np.asarray(a, dtype=np.float32).reshape(-1).astype(np.float64) - ref)
        ratio = np.where(np.isfinite(err), err, np.inf) / bar
        worst[name] = float(ratio.max()) if ratio.size else 0.0
        note("adam fp64", f"{label} {name}: worst share of the counted bar", worst[name], 1.0)
        assert worst[name] <= 1.0, f"{label}: {name} off by {worst[name]:.3g} of its counted bar at flat index {int(ratio.argmax())}"
    return worst


def torch_p_error_ulp(p_got, p_torch, p_old):
    """|p - p_torch| in units of max(ulp(p_new), ulp(update)), update = p_torch - p_old as float64"""
    p_got, p_torch, p_old = (np.asarray(t, dtype=np.float32).astype(np.float64).reshape(-1) for t in (p_got, p_torch, p_old))
    unit = np.maximum(ulp32(p_torch), ulp32(p_torch - p_old))
    return np.abs(p_got - p_torch) / unit


def check_against_torch(got, torch_state, p_old, label):
    """got, torch_state = (p, m, v): moments bit for bit, parameters within TORCH_P_BAR_ULP -> worst parameter error in that unit"""
    check_bits(got[1], torch_state[1], f"{label} exp_avg against torch.optim.Adam")
    check_bits(got[2], torch_state[2], f"{label} exp_avg_sq against torch.optim.Adam")
    e = torch_p_error_ulp(got[0], torch_state[0], p_old)
    worst = float(e.max()) if e.size else 0.0
    note("adam torch", f"{label} parameters, units of max(ulp(p), ulp(update))", worst, TORCH_P_BAR_ULP)
    assert worst <= TORCH_P_BAR_ULP, f"{label}: parameters off by {worst:.3g} units at flat index {int(e.argmax())}"
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the weight images, from the layouts documented in include/vqseg.h and csrc/conv_pack.hip
# ---------------------------------------------------------------------------------------------------------------------
def _hi_lo(w):
    w = np.asarray(w, dtype=np.float32)
    hi = bf16_bits(w)
    return hi, bf16_bits((w - bf16_to_f32(hi)).astype(np.float32))


def _pad32(a):
    """zero-pad the last axis to a multiple of 32"""
    return np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, -a.shape[-1] % 32)])


def image_fwd(w, lo=False, defect=None):
    """[Cout][KH][KW][Cin^32]: the weight with the input channel innermost.  defect: 'lo_of_v', 'pad_unwritten'"""
    hi, low = _hi_lo(w)
    if defect == "lo_of_v":
        low = bf16_bits(w)
    out = _pad32((low if lo else hi).transpose(0, 2, 3, 1))
    if defect == "pad_unwritten" and w.shape[1] % 32:
        out[..., w.shape[1]:] = I16_FILL
    return out.reshape(-1)


def image_tr(w, lo=False, defect=None):
    """[Cin][KH][KW flipped][Cout^32]: both tap axes reversed, the output channel innermost.  defect: 'no_flip'"""
    hi, low = _hi_lo(w)
    src = low if lo else hi
    if defect != "no_flip":
        src = src[:, :, ::-1, ::-1]
    return _pad32(src.transpose(1, 2, 3, 0)).reshape(-1)


def image_s3(w, c1, defect=None):
    """[Cout][KH][KW][3 Cin]: per concat segment (channels [0, c1), then [c1, Cin)) the channel runs [hi | hi | lo].
    defect: 'second_segment' (its block is laid out with the FIRST segment's width)"""
    hi, low = (a.transpose(0, 2, 3, 1) for a in _hi_lo(w))
    cin = w.shape[1]
    segs = [(0, c1)] + ([(c1, cin)] if c1 < cin else [])
    if defect == "second_segment" and c1 < cin:
        out = np.full(hi.shape[:3] + (3 * cin,), I16_FILL, dtype=np.uint16)
        out[..., :3 * c1] = np.concatenate([hi[..., :c1], hi[..., :c1], low[..., :c1]], axis=-1)
        for part, src in enumerate((hi, hi, low)):                    # stride c1 between the parts instead of Cin - c1
            lo_, n = 3 * c1 + part * c1, cin - c1
            n = max(0, min(n, 3 * cin - lo_))
            out[..., lo_:lo_ + n] = src[..., c1:c1 + n]
        return out.reshape(-1)
    return np.concatenate([np.concatenate([hi[..., a:b], hi[..., a:b], low[..., a:b]], axis=-1) for a, b in segs], axis=-1).reshape(-1)


def image_s2(w, lo=False, defect=None):
    """stride-2 data-gradient sub-images of a K x K weight (K = 1 or 3), classes (0,0), (0,1), (1,0), (1,1) one after the other:
    along each axis an even class holds the forward taps (2, 0) in that order, an odd class the tap (1); each sub-image is
    [Cin][th][tw][Cout^32].  K = 1: the single tap.  defect: 'window_order' (even classes hold (0, 2))"""
    hi, low = _hi_lo(w)
    src = low if lo else hi
    k = w.shape[2]
    if k == 1:
        return _pad32(src.transpose(1, 2, 3, 0)).reshape(-1)
    even = [0, 2] if defect == "window_order" else [2, 0]
    parts = []
    for ph in (0, 1):
        for pw in (0, 1):
            sub = src[:, :, even if ph == 0 else [1], :][:, :, :, even if pw == 0 else [1]]
            parts.append(_pad32(sub.transpose(1, 2, 3, 0)).reshape(-1))
    return np.concatenate(parts)


def fwd_elems(cout, cin, kh, kw):
    return cout * kh * kw * ((cin + 31) // 32 * 32)


def tr_elems(cout, cin, kh, kw):
    return cin * kh * kw * ((cout + 31) // 32 * 32)


def check_image(got, want, label, padding=None):
    """uint16 images equal bit for bit; `padding` (a boolean mask over the image) must hold zeros -- reported first, since an unwritten
    padding element is its own defect"""
    got, want = np.asarray(got).reshape(-1).view(np.uint16), np.asarray(want, dtype=np.uint16).reshape(-1)
    assert got.shape == want.shape, f"{label}: {got.size} elements against {want.size}"
    if padding is not None:
        pad = np.asarray(padding).reshape(-1)
        assert (want[pad] == 0).all()
        assert (got[pad] == 0).all(), f"{label}: {int((got[pad] != 0).sum())} padding elements are not zero (first value {got[pad][got[pad] != 0][0]:#06x})"
    bad = got != want
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{label}: {i.size} of {got.size} image elements differ from the NumPy layout; first at {i[0]} "
                             f"(got {got[i[0]]:#06x}, expected {want[i[0]]:#06x}), last at {i[-1]}")


def padding_mask(rows, c):
    """mask over a [rows][c^32] image: True on the channels c .. c^32 - 1"""
    cp = (c + 31) // 32 * 32
    return np.tile(np.arange(cp) >= c, rows)


def check_lo_property(w, hi_bits, lo_bits, label):
    """float(hi) + float(lo) reproduces w within 2^-16 relative on normal values (hi keeps 8 significant bits, lo the next 8)"""
    w = np.asarray(w, dtype=np.float32).astype(np.float64).reshape(-1)
    rec = bf16_to_f32(hi_bits).astype(np.float64).reshape(-1) + bf16_to_f32(lo_bits).astype(np.float64).reshape(-1)
    ok = np.abs(w) >= 2.0 ** -100
    err = float((np.abs(rec - w)[ok] / np.abs(w)[ok]).max()) if ok.any() else 0.0
    note("pack", f"{label} |hi + lo - w| / |w|", err, 2.0 ** -16)
    assert err <= 2.0 ** -16, f"{label}: hi + lo misses w by {err:.3e} relative"


def weight(seed, shape):
    """a weight whose values need their low bits (not bf16-exact), mixed signs, magnitudes over three decades"""
    rs = np.random.RandomState(seed)
    return (rs.uniform(-1, 1, size=shape) * 10.0 ** rs.randint(-3, 0, size=shape)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# work items
# ---------------------------------------------------------------------------------------------------------------------
def work_items(numel, k, cout, cin):
    """the tiles of one parameter: 32 x 32 channel tiles for k = 3, 32 x 128 for k = 1, chunks of 4096 elements otherwise"""
    if numel <= 0:
        return 0
    if k == 3:
        return -(-cout // 32) * -(-cin // 32)
    if k == 1:
        return -(-cout // 32) * -(-cin // 128)
    return -(-numel // ADAM_CHUNK)


# ---------------------------------------------------------------------------------------------------------------------
# guarded device buffers and the launch table (torch and the library are imported here, not at module level)
# ---------------------------------------------------------------------------------------------------------------------
class Guarded:
    """one device allocation [GUARD sentinels | shift | n payload words | GUARD sentinels]; float32 or int16 words.  The payload starts
    16-byte aligned plus `shift` words."""

    def __init__(self, device, n, dtype="f32", shift=0, values=None):
        import torch
        self.n, self.shift, self.f32 = int(n), int(shift), dtype == "f32"
        tdt, self.sent = (torch.int32, F32_SENTINEL) if self.f32 else (torch.int16, I16_SENTINEL)
        self.raw = torch.full((GUARD + shift + self.n + GUARD,), self.sent, dtype=tdt, device=device)
        assert self.raw.data_ptr() % 16 == 0
        self.lo = GUARD + shift
        body = self.raw[self.lo:self.lo + self.n]
        if values is not None:
            v = np.ascontiguousarray(values, dtype=np.float32 if self.f32 else np.uint16).reshape(-1)
            assert v.size == self.n
            body.copy_(torch.from_numpy(v.view(np.int32 if self.f32 else np.int16).copy()))
        elif not self.f32:
            body.fill_(I16_FILL)
        self.ptr = self.raw.data_ptr() + self.lo * (4 if self.f32 else 2)

    def get(self):
        a = self.raw[self.lo:self.lo + self.n].cpu().numpy()
        return a.view(np.float32).copy() if self.f32 else a.view(np.uint16).copy()

    def guards_intact(self):
        a = self.raw.cpu().numpy().astype(np.int64) & (0xFFFFFFFF if self.f32 else 0xFFFF)
        return bool((a[:self.lo] == self.sent).all() and (a[self.lo + self.n:] == self.sent).all())


class AdamParam:
    """one record of the launch table with its guarded buffers.  k = 0: flat; k = 1 / 3: a [cout][cin][k][k] weight with the images named
    in `images` (a subset of 'fwd', 'tr', 's3').  shift = {'p': 1, ...}: that pointer is offset by one float from 16-byte alignment."""

    def __init__(self, device, state, k=0, cout=0, cin=0, c1=0, images=(), shift=None):
        shift = shift or {}
        self.state = tuple(np.ascontiguousarray(t, dtype=np.float32).reshape(-1) for t in state)
        self.numel = self.state[0].size
        self.k, self.cout, self.cin, self.c1 = k, cout, cin, (c1 or cin)
        assert k == 0 or self.numel == cout * cin * k * k
        self.buf = {name: Guarded(device, self.numel, "f32", shift.get(name, 0), values) for name, values in zip("pgmv", self.state)}
        sizes = {"fwd": fwd_elems(cout, cin, k, k), "tr": tr_elems(cout, cin, k, k), "s3": cout * k * k * 3 * cin} if k else {}
        self.img = {name: Guarded(device, sizes[name], "i16") for name in images}

    def record(self, rec):
        for name in "pgmv":
            rec[name] = self.buf[name].ptr
        rec["numel"], rec["k"], rec["cout"], rec["cin"], rec["c1"] = self.numel, self.k, self.cout, self.cin, self.c1
        for name, b in self.img.items():
            rec[name] = b.ptr

    def n_items(self):
        return work_items(self.numel, self.k, self.cout, self.cin)

    def results(self):
        return tuple(self.buf[name].get() for name in "pmv")

    def guards_intact(self):
        return all(b.guards_intact() for b in list(self.buf.values()) + list(self.img.values()))

    def untouched(self):
        """every payload still holds what it was given (the refused calls)"""
        same = all((f32_bits(self.buf[name].get()) == f32_bits(s)).all() for name, s in zip("pgmv", self.state))
        return same and all((b.get() == I16_FILL).all() for b in self.img.values())


def adam_items(params, order="sorted", seed=0):
    """[n_items][2] int32 (parameter, tile): every tile of every parameter once; 'sorted', 'reversed' or 'shuffled' (seeded)"""
    rows = [(i, t) for i, p in enumerate(params) for t in range(p.n_items())]
    items = np.array(rows, dtype=np.int32).reshape(-1, 2)
    if order == "reversed":
        items = items[::-1]
    elif order == "shuffled":
        items = items[np.random.RandomState(seed).permutation(items.shape[0])]
    else:
        assert order == "sorted"
    return np.ascontiguousarray(items)


def adam_launch(params, items, hyper, null_params=False, null_items=False, n_items=None):
    """vqseg_adam_step_f32 on the table of `params` -> its return code (synchronised)"""
    import torch
    from vq_seg_amd import _hip
    from vq_seg_amd.optim import _REC
    L = _hip.lib()
    dev = params[0].buf["p"].raw.device
    rec = np.zeros(len(params), dtype=_REC)
    for i, p in enumerate(params):
        p.record(rec[i])
    rec_d = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    items_d = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32).reshape(-1).copy() if len(items) else np.zeros(2, dtype=np.int32)).to(dev)
    lr, b1, b2, eps, step = hyper
    n = int(len(items)) if n_items is None else n_items
    rc = L.vqseg_adam_step_f32(None if null_params else rec_d.data_ptr(), None if null_items else items_d.data_ptr(), n, float(lr), float(b1),
                               float(b2), float(eps), int(step), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


# ---------------------------------------------------------------------------------------------------------------------
# the cases both test modules use
# ---------------------------------------------------------------------------------------------------------------------
HYPER = (3e-3, 0.9, 0.999, 1e-8, 3)                                   # lr, beta1, beta2, eps, step
FLAT_NUMELS = (1, 3, 4, 5, 1023, 1024, 1027, 4095, 4096, 4097, 8195)
K3_SHAPES = ((1, 1), (31, 8), (33, 24), (40, 33), (64, 64), (32, 192))       # (Cout, Cin): 32 x 32 tiles
K1_SHAPES = ((1, 1), (33, 127), (32, 128), (40, 129), (96, 200), (64, 256))  # 32 x 128 tiles
VALUE_STEPS = (1, 2, 1000, 10 ** 7)
VALUE_BETAS = ((0.9, 0.999), (0.0, 0.0), (0.5, 0.9999))
# vqseg_adam_work_items, written out: (numel, k, cout, cin) -> tiles
WORK_ITEM_COUNTS = {
    (0, 0, 0, 0): 0, (1, 0, 0, 0): 1, (4096, 0, 0, 0): 1, (4097, 0, 0, 0): 2, (8195, 0, 0, 0): 3,
    (0, 3, 0, 0): 0, (9, 3, 1, 1): 1, (31 * 8 * 9, 3, 31, 8): 1, (33 * 24 * 9, 3, 33, 24): 2, (40 * 33 * 9, 3, 40, 33): 4,
    (64 * 64 * 9, 3, 64, 64): 4, (32 * 192 * 9, 3, 32, 192): 6,
    (1, 1, 1, 1): 1, (33 * 127, 1, 33, 127): 2, (32 * 128, 1, 32, 128): 1, (40 * 129, 1, 40, 129): 4, (96 * 200, 1, 96, 200): 6,
    (64 * 256, 1, 64, 256): 4,
}


def flat_state(n):
    return adam_data(500 + n, n)


def tile_state(k, cout, cin):
    return adam_data(600 + 7 * k + 13 * cout + cin, cout * cin * k * k)


def s3_splits(cin):
    """the concat splits the split-3 image is checked at (cin % 32 == 0)"""
    return sorted({32, cin - 32, cin} - {0})


def expected_images(p_new, k, cout, cin, c1, images):
    if not images:
        return {}
    w = np.asarray(p_new, dtype=np.float32).reshape(cout, cin, k, k)
    make = {"fwd": lambda: image_fwd(w), "tr": lambda: image_tr(w), "s3": lambda: image_s3(w, c1)}
    return {name: make[name]() for name in images}


def image_padding(name, k, cout, cin):
    if name == "fwd":
        return padding_mask(cout * k * k, cin)
    if name == "tr":
        return padding_mask(cin * k * k, cout)
    return None
