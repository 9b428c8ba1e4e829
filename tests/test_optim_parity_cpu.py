"""tests/optim_cases.py held to account without a GPU: the float32 emulation of `adam_one` against rational arithmetic and against
torch.optim.Adam on the CPU, the NumPy image layouts against loops written from the documented layouts and against each other, the
counted float64 bars on every case the GPU suite runs, and -- the point of this module -- every assertion function against an
emulation that carries ONE defect: each defect must trip the assertion meant for it, so the GPU suite would fail on a kernel that is
subtly wrong in that way."""
import os
import re

import numpy as np
import pytest
import torch

from tests import optim_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_constants_are_those_of_the_source():
    assert int(re.search(r"#define VQSEG_ADAM_CHUNK (\d+)", _read("include", "vqseg.h")).group(1)) == C.ADAM_CHUNK
    pack = _read("vq_seg_amd", "csrc", "conv_pack.hip")
    assert pack.count("if (blocks > 4096) blocks = 4096;") == 3 and pack.count("__launch_bounds__(256)") >= 3
    assert C.PACK_GRID_CAP == 4096 * 256
    for (numel, k, cout, cin), want in C.WORK_ITEM_COUNTS.items():
        assert C.work_items(numel, k, cout, cin) == want


# ------------------------------------------------------------------------------------------------ the exact fma
def test_fma32_rounds_once():
    """against rational arithmetic: random operands over many binades, cancelling sums, subnormal results, and constructed products
    whose float64 sum lands EXACTLY on a float32 midpoint while the exact sum does not (where float64-then-cast rounds twice)"""
    rs = np.random.RandomState(1)
    n = 3000
    a = (rs.uniform(-2, 2, n) * 2.0 ** rs.randint(-30, 30, n)).astype(np.float32)
    b = (rs.uniform(-2, 2, n) * 2.0 ** rs.randint(-30, 30, n)).astype(np.float32)
    c = (rs.uniform(-2, 2, n) * 2.0 ** rs.randint(-40, 40, n)).astype(np.float32)
    c[:500] = (-(a[:500].astype(np.float64) * b[:500])).astype(np.float32)          # cancellation: the result is the product's tail
    a[500:700] *= np.float32(2.0 ** -70)                                             # subnormal and underflowing results
    c[500:700] = (rs.uniform(-4, 4, 200) * 2.0 ** -140).astype(np.float32)
    one_up, one_dn = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23)          # product 1 - 2^-46: just below one
    ties = []
    for sign in (1.0, -1.0):
        for e in (-4, 0, 7):                                                          # c = 2^(e + 24) (+ one ulp): half an ulp is 2^e
            for odd in (0.0, 1.0):
                for x, y in ((one_up, one_dn), (one_up, one_up)):                     # a b = 2^e (1 -+ ...): below / above the midpoint
                    ties.append((sign * x * np.float32(2.0 ** e), y, sign * np.float32(2.0 ** (e + 24) + odd * 2.0 ** (e + 1))))
    ta, tb, tc = (np.array(t, dtype=np.float32) for t in zip(*ties))
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = C.fma32(a, b, c)
    want = np.array([C.fma32_fraction(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    C.check_bits(got, want, "fma32 against rational arithmetic")
    # the constructed ties are double-rounding cases: float64-then-cast gets some of them wrong, which is why it is not used
    naive = (ta.astype(np.float64) * tb.astype(np.float64) + tc.astype(np.float64)).astype(np.float32)
    assert (C.f32_bits(naive) != C.f32_bits(want[n:])).any()


def test_rational_rounding_to_float32():
    from fractions import Fraction as Fr
    f = np.float32
    assert C.round_fraction_f32(Fr(1) + Fr(1, 2 ** 24)) == f(1.0)                                  # tie to even, down
    assert C.round_fraction_f32(Fr(1) + Fr(3, 2 ** 24)) == f(1 + 2.0 ** -22)                       # tie to even, up
    assert C.round_fraction_f32(Fr(1) + Fr(1, 2 ** 24) + Fr(1, 2 ** 90)) == f(1 + 2.0 ** -23)
    assert C.round_fraction_f32(Fr(1, 2 ** 150)) == f(0.0) and C.round_fraction_f32(Fr(3, 2 ** 150)) == f(2.0 ** -148)
    assert C.round_fraction_f32(-Fr(1, 2 ** 149)) == f(-2.0 ** -149)
    assert np.isinf(C.round_fraction_f32(Fr(2) ** 128 - Fr(2) ** 103)) and C.round_fraction_f32(Fr(2) ** 128 - Fr(2) ** 103 - 1) == np.finfo(f).max


def test_emulation_through_rational_arithmetic_on_the_special_values():
    """the whole chain at the special-value tensor (subnormals, underflowing and overflowing squares): the two fmas recomputed through
    Fractions wherever their operands are finite"""
    p, g, m, v = C.special_values()
    for b1, b2 in C.VALUE_BETAS:
        s = C.adam_scalars(3e-3, b1, b2, 1e-8, 2)
        _, m1, v1 = C.adam_emulate(p, g, m, v, 3e-3, b1, b2, 1e-8, 2)
        with np.errstate(all="ignore"):
            d = (g - m).astype(np.float32)
            ag, vb = (s["a2"] * g).astype(np.float32), (v * s["b2"]).astype(np.float32)
        fin = np.flatnonzero(np.isfinite(d) & np.isfinite(ag) & np.isfinite(vb) & np.isfinite(g))
        C.check_bits(m1[fin], np.array([C.fma32_fraction(s["w1"], d[i], m[i]) for i in fin]), "m through Fractions")
        C.check_bits(v1[fin], np.array([C.fma32_fraction(ag[i], g[i], vb[i]) for i in fin]), "v through Fractions")


# ------------------------------------------------------------------------------------------------ emulation against torch
def test_emulation_against_torch_adam_on_the_cpu():
    """6 steps x 200 000 elements, gradients over five decades plus exact zeros; every step starts the emulation from torch's own state
    (no accumulation): both moments bit for bit, parameters within twice the measured worst error (printed; profiles/optim_parity.md)"""
    n = 200_000
    p0, _, _, _ = C.adam_data(9, n)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([q], lr=3e-3, betas=(0.9, 0.999), foreach=False, fused=False)
    worst = 0.0
    for step in range(1, 7):
        lr = 3e-3 * (1.0 - 0.1 * (step - 1))
        opt.param_groups[0]["lr"] = lr
        g = C.adam_data(20 + step, n)[1]
        st = opt.state[q]
        before = (q.detach().numpy().copy(), g, st["exp_avg"].numpy().copy() if st else np.zeros(n, np.float32),
                  st["exp_avg_sq"].numpy().copy() if st else np.zeros(n, np.float32))
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[q]
        got = C.adam_emulate(*before, lr, 0.9, 0.999, 1e-8, step)
        worst = max(worst, C.check_against_torch(got, (q.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), before[0],
                                                 f"step {step}"))
    C.note("adam torch", "worst over the 6 steps (the measured figure behind TORCH_P_MEASURED_ULP)", worst, C.TORCH_P_MEASURED_ULP)
    assert C.TORCH_P_BAR_ULP == 2 * C.TORCH_P_MEASURED_ULP


# ------------------------------------------------------------------------------------------------ the float64 bars
def _all_ordinary_states():
    for n in C.FLAT_NUMELS:
        yield f"flat {n}", C.flat_state(n)
    for k, shapes in ((3, C.K3_SHAPES), (1, C.K1_SHAPES)):
        for cout, cin in shapes:
            yield f"k{k} {cout}x{cin}", C.tile_state(k, cout, cin)


def test_counted_bars_hold_for_the_emulation_and_undercut_the_old_max_norm_bars():
    """every ordinary case of the GPU suite: the emulation lies within the counted per-element bars of the float64 step, and each bar
    lies below the 2.5e-7 / 1e-7 of scale that tests/test_optim_gpu.py asserts"""
    for label, state in _all_ordinary_states():
        got = C.adam_emulate(*state, *C.HYPER)
        C.check_adam_fp64(got, state, C.HYPER, label)


def test_ulp32():
    x = np.array([1.0, 1.5, 2.0, 0.75, 2.0 ** -126, 2.0 ** -130, 0.0, -3.0])
    assert (C.ulp32(x) == np.array([2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -24, 2.0 ** -149, 2.0 ** -149, 2.0 ** -149, 2.0 ** -22])).all()


# ------------------------------------------------------------------------------------------------ one defect each: Adam
def _trips(fn, match):
    with pytest.raises(AssertionError, match=match):
        fn()


@pytest.mark.parametrize("defect,tripped", [
    ("m_unfused", " m against the float32 emulation"), ("v_unfused", " v against the float32 emulation"),
    ("bc2_inside_sqrt", " p against the float32 emulation"), ("eps_before_div", " p against the float32 emulation")])
def test_a_defect_in_the_adam_arithmetic_trips_the_bit_comparison(defect, tripped):
    state = C.flat_state(4097)
    bad = C.adam_emulate(*state, *C.HYPER, defect=defect)
    _trips(lambda: C.check_adam_emulation(bad, state, C.HYPER, defect), tripped)
    good = C.adam_emulate(*state, *C.HYPER)
    C.check_adam_emulation(good, state, C.HYPER, "no defect")
    untouched = {"m_unfused": "v", "v_unfused": "m"}.get(defect, "mv")      # and what the defect does not reach keeps its bits
    for name, a, b in zip("pmv", bad, good):
        if name in untouched:
            assert (C.f32_bits(a) == C.f32_bits(b)).all(), (defect, name)


def test_an_unfused_moment_stays_inside_the_old_max_norm_bar():
    """why the bit comparison is needed: splitting either fma is invisible to `largest difference / largest magnitude <= 1e-7`"""
    state = C.flat_state(4097)
    good = C.adam_emulate(*state, *C.HYPER)
    for defect, i in (("m_unfused", 1), ("v_unfused", 2)):
        bad = C.adam_emulate(*state, *C.HYPER, defect=defect)
        rel = np.abs(bad[i].astype(np.float64) - good[i]).max() / np.abs(good[i].astype(np.float64)).max()
        assert 0 < rel <= C.OLD_MOMENT_BAR


@pytest.mark.parametrize("n", [5, 1027, 4097])
def test_a_skipped_last_element_trips_the_bit_comparison_and_the_float64_bar(n):
    state = C.flat_state(n)
    state[1][-1] = np.float32(0.37)                                       # a gradient there, so a skipped update shows
    bad = C.adam_emulate(*state, *C.HYPER, defect="skip_last")
    _trips(lambda: C.check_adam_emulation(bad, state, C.HYPER, "skip_last"), rf"first at {n - 1} ")
    _trips(lambda: C.check_adam_fp64(bad, state, C.HYPER, "skip_last"), rf"counted bar at flat index {n - 1}")


def test_special_values_are_all_there_and_the_emulation_keeps_ieee_semantics():
    p, g, m, v = C.special_values()
    assert 4000 <= p.size <= 4200
    sub = lambda a: (np.abs(a) > 0) & (np.abs(a) < 2.0 ** -126)
    with np.errstate(all="ignore"):
        g2 = g.astype(np.float32) * g
    assert np.isnan(g).any() and np.isposinf(g).any() and np.isneginf(g).any() and sub(g).any() and sub(m).any() and sub(v).any()
    assert ((g2 == 0) & (g != 0)).any() and (np.isinf(g2) & np.isfinite(g)).any() and (v == 0).any()
    for a in (g, m, p):
        assert (C.f32_bits(a) == 0x80000000).any() and (C.f32_bits(a) == 0).any()
    p1, m1, v1 = C.adam_emulate(p, g, m, v, 3e-3, 0.9, 0.999, 0.0, 1)
    assert np.isnan(p1).any() and sub(m1).any() and sub(v1).any() and (C.f32_bits(p1) == 0x80000000).any()
    # flushing subnormals to zero -- what a kernel built with denormals off would do -- is caught by bits
    ftz = tuple(np.where(sub(a), np.copysign(np.float32(0), a), a).astype(np.float32) for a in (p1, m1, v1))
    _trips(lambda: C.check_adam_emulation(ftz, (p, g, m, v), (3e-3, 0.9, 0.999, 0.0, 1), "ftz"), "against the float32 emulation")
    # a NaN that went missing is caught by position
    lost = (np.where(np.isnan(p1), np.float32(0), p1), m1, v1)
    _trips(lambda: C.check_adam_emulation(lost, (p, g, m, v), (3e-3, 0.9, 0.999, 0.0, 1), "nan"), "NaN positions differ")


# ------------------------------------------------------------------------------------------------ the image layouts
def _loops(w, kind, c1=None):
    """the documented layouts by explicit loops over (co, ci, kh, kw) -- slow, tiny shapes only -- as (hi, lo) uint16"""
    cout, cin, kh, kw = w.shape
    hi_of = lambda x: int(C.bf16_bits(np.float32(x)).reshape(-1)[0])
    lo_of = lambda x: hi_of(np.float32(x) - C.bf16_to_f32(np.uint16(hi_of(x))).reshape(-1)[0])
    cin_p, cout_p = -(-cin // 32) * 32, -(-cout // 32) * 32
    if kind == "fwd":
        hi, lo = np.zeros((cout, kh, kw, cin_p), np.uint16), np.zeros((cout, kh, kw, cin_p), np.uint16)
    elif kind == "tr":
        hi, lo = np.zeros((cin, kh, kw, cout_p), np.uint16), np.zeros((cin, kh, kw, cout_p), np.uint16)
    else:
        hi, lo = np.zeros((cout, kh, kw, 3 * cin), np.uint16), None
    for co in range(cout):
        for ci in range(cin):
            for a in range(kh):
                for b in range(kw):
                    x = w[co, ci, a, b]
                    if kind == "fwd":
                        hi[co, a, b, ci], lo[co, a, b, ci] = hi_of(x), lo_of(x)
                    elif kind == "tr":
                        hi[ci, kh - 1 - a, kw - 1 - b, co], lo[ci, kh - 1 - a, kw - 1 - b, co] = hi_of(x), lo_of(x)
                    else:
                        first = ci < c1
                        width, start, loc = (c1, 0, ci) if first else (cin - c1, 3 * c1, ci - c1)
                        hi[co, a, b, start + loc] = hi[co, a, b, start + width + loc] = hi_of(x)
                        hi[co, a, b, start + 2 * width + loc] = lo_of(x)
    return hi.reshape(-1), (None if lo is None else lo.reshape(-1))


def test_numpy_layouts_against_loops_over_the_documented_index_order():
    for shape in ((3, 5, 3, 3), (2, 3, 1, 3), (33, 2, 1, 1), (2, 34, 3, 3)):
        w = C.weight(sum(shape), shape)
        for kind, fn in (("fwd", C.image_fwd), ("tr", C.image_tr)):
            hi, lo = _loops(w, kind)
            C.check_image(fn(w), hi, f"{kind} hi {shape}")
            C.check_image(fn(w, lo=True), lo, f"{kind} lo {shape}")
    for shape, c1 in (((2, 64, 3, 3), 32), ((2, 64, 1, 1), 64), ((3, 96, 1, 1), 64)):
        w = C.weight(sum(shape) + c1, shape)
        C.check_image(C.image_s3(w, c1), _loops(w, "s3", c1)[0], f"s3 {shape} c1 {c1}")
    # stride 2: the gradient of y[o] = sum_k xp[2 o + k] w[k] reaches an even padded row 2 i from (o, k) = (i - 1, 2), (i, 0) -- window
    # order (2, 0) -- and an odd row from (i, 1): per class a data-gradient image WITHOUT a flip of those taps
    w = C.weight(5, (3, 4, 3, 3))
    hi = C.bf16_bits(w)
    off = 0
    got = C.image_s2(w)
    for ph in (0, 1):
        for pw in (0, 1):
            th, tw = ([2, 0], [1])[ph], ([2, 0], [1])[pw]
            for ci in range(4):
                for a in th:
                    for b in tw:
                        assert (got[off:off + 3] == hi[:, ci, a, b]).all() and (got[off + 3:off + 32] == 0).all()
                        off += 32
    assert off == got.size == 4 * 9 * 32
    assert (C.image_s2(C.weight(6, (33, 2, 1, 1))) == C.image_tr(C.weight(6, (33, 2, 1, 1)))).all()


def test_layout_properties_padding_flip_segments_and_classes():
    w = C.weight(3, (40, 24, 3, 3))
    fwd, tr = C.image_fwd(w).reshape(40, 3, 3, 32), C.image_tr(w).reshape(24, 3, 3, 64)
    assert (fwd[..., 24:] == 0).all() and (tr[..., 40:] == 0).all() and (C.image_fwd(w, lo=True).reshape(40, 3, 3, 32)[..., 24:] == 0).all()
    # the data-gradient image is the forward image of the transposed, tap-reversed weight
    assert (C.image_tr(w) == C.image_fwd(np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]))).all()
    assert (tr[:, 0, 0, :40] == fwd[:, 2, 2, :24].T).all() and (tr[:, 1, 1, :40] == fwd[:, 1, 1, :24].T).all()
    # split-3 with the split at Cin is [hi | hi | lo] of the whole row; with a split, each segment on its own
    w = C.weight(4, (8, 96, 3, 3))
    hi, lo = C.image_fwd(w).reshape(8, 3, 3, 96), C.image_fwd(w, lo=True).reshape(8, 3, 3, 96)
    assert (C.image_s3(w, 96).reshape(8, 3, 3, 288) == np.concatenate([hi, hi, lo], -1)).all()
    s3 = C.image_s3(w, 64).reshape(8, 3, 3, 288)
    assert (s3[..., :192] == np.concatenate([hi[..., :64]] * 2 + [lo[..., :64]], -1)).all()
    assert (s3[..., 192:] == np.concatenate([hi[..., 64:]] * 2 + [lo[..., 64:]], -1)).all()
    # the four stride-2 classes partition the nine taps; the (1, 1) class is the centre tap alone
    w = C.weight(5, (40, 24, 3, 3))
    s2 = C.image_s2(w)
    assert s2.size == 24 * 9 * 64 and sorted(s2.tolist()) == sorted(C.image_tr(w).tolist())
    assert (s2[-24 * 64:].reshape(24, 64) == C.image_tr(w).reshape(24, 3, 3, 64)[:, 1, 1]).all()
    C.check_lo_property(w, C.bf16_bits(w), C._hi_lo(w)[1], "reference hi / lo")


@pytest.mark.parametrize("defect,fn,args,tripped", [
    ("no_flip", "image_tr", dict(), "image elements differ"),
    ("lo_of_v", "image_fwd", dict(lo=True), "image elements differ"),
    ("second_segment", "image_s3", dict(c1=32), "image elements differ"),
    ("window_order", "image_s2", dict(), "image elements differ"),
    ("pad_unwritten", "image_fwd", dict(), "padding elements are not zero"),
])
def test_a_defect_in_an_image_layout_trips_the_comparison(defect, fn, args, tripped):
    shape = (40, 96, 3, 3) if defect == "second_segment" else (40, 24, 3, 3)
    w = C.weight(11, shape)
    f = getattr(C, fn)
    want, bad = f(w, **args), f(w, defect=defect, **args)
    pad = C.padding_mask(40 * 9, shape[1]) if fn == "image_fwd" else None
    C.check_image(want, want, "no defect", padding=pad)
    _trips(lambda: C.check_image(bad, want, defect, padding=pad), tripped)
    if defect == "lo_of_v":
        _trips(lambda: C.check_lo_property(w, C.image_fwd(w)[~pad], bad[~pad], defect), "hi \\+ lo misses w")
    if defect == "no_flip":                                              # a 1 x 1 kernel has nothing to flip: the defect needs k = 3
        w1 = C.weight(12, (40, 24, 1, 1))
        assert (C.image_tr(w1, defect=defect) == C.image_tr(w1)).all()
