"""Direct parity of the stem and reflect-fold kernels through the C ABI against the float64 references of tests/stem_cases.py:

  A  vqseg_stem7_conv_f      stem7_fused_kernel<false / true> (conv_igemm.hip): raw output + BatchNorm partials, the bf16 affine
                             epilogue, the split-3 epilogue, at one / two / three strips per row, odd extents and the smallest image
  B  vqseg_im2col_f          im2col_stem7_strip_kernel<..>, im2col_stem7_kernel<..>, im2col_stem_kernel<..>: every output form, bit for bit
  C  vqseg_reflect_fold_f    reflect_fold_kernel<bf16, 8 / 1>, <float, 4 / 1>
  D  vqseg_reflect_ring_f    the ring convolution + reflect_ring_fold_kernel<bf16, 8>

Outputs and statistics are pre-filled with NaN and followed by guard rows that must keep their fill; references are built from the
values the kernels receive; the bounds are derived in stem_cases.py (tests/test_stem_bound_cpu.py shows without a GPU that a correct
kernel meets them and which mistakes they catch).  The only bars not derived there are quoted from existing tests: 1e-5 / 1e-4 for
the BatchNorm statistics, 3e-5 for the split-3 stem against the true operation, half a bf16 ulp in test_nn_kernels_gpu.check."""
import pytest
import torch
from torch import nn

from tests import stem_cases as sc
from tests import synth
from tests.test_dispatch_variants_gpu import _assert_batchnorm_statistics_of
from tests.test_nn_kernels_gpu import BF16, F32, check, option

pytestmark = pytest.mark.gpu

GUARD = 2                                                       # rows / slots behind each buffer


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def lib():
    from vq_seg_amd import _hip
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def nan_rows(rows, width, dtype):
    return torch.full((rows, width), float("nan"), dtype=dtype, device=dev())


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def still_nan_fill(t):
    return torch.equal(bits(t), bits(torch.full_like(t, float("nan"))))


def assert_inside(got, want, limit, what):
    """every element of got within limit of want; prints the largest share of the bound in use before it asserts"""
    share = ((got.cpu().double() - want).abs() / limit.clamp_min(1e-300)).nan_to_num(float("inf")).max().item()
    print(f"{what}: {share:.3f} of the bound")
    bad = sc.outside(got.cpu(), want, limit)
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} elements outside the bound, first at {i}: got {float(got.cpu()[i])!r}, "
                             f"reference {float(want[i])!r}, bound {float(limit[i]):.3e}")


# ---------------------------------------------------------------------------------------------------------------------------
# A. vqseg_stem7_conv_f
# ---------------------------------------------------------------------------------------------------------------------------
STEM = [(c, r) for c in sorted(sc.STEM_CASES) for r in (False, True)]
STEM_IDS = [f"{c}-{'reflect' if r else 'zero'}" for c, r in STEM]
_STEM_DEVICE = {}


def _stem_device(case):
    """(image, bf16 weight image, split-3 weight image, scale, shift) on the GPU, uploaded once"""
    if case not in _STEM_DEVICE:
        x, wt = sc.stem_operands(case)
        scale, shift = sc.stem_affine()
        _STEM_DEVICE[case] = (x.to(dev()), sc.stem_weight_image(wt, False).to(dev()), sc.stem_weight_image(wt, True).to(dev()),
                              scale.to(dev()), shift.to(dev()))
    return _STEM_DEVICE[case]


def _stem(case, reflect, s3=False, affine=False, relu=0):
    """one launch: (y [M, 64] bf16 or [M, 128] = hi | lo, statistics slots or None); asserts the guards behind both"""
    L = lib()
    n, h, w = sc.STEM_CASES[case]
    ho, wo = sc.stem_out_size(h, w)
    m = n * ho * wo
    x, img, img3, scale, shift = _stem_device(case)
    y = nan_rows(m + GUARD, 128 if s3 else 64, BF16)
    stat = None
    if not affine:
        stat = torch.full((L.vqseg_conv_stat_slots(m, 64) + GUARD, 2, 64), float("nan"), dtype=F32, device=dev())
    rc = L.vqseg_stem7_conv_f(int(s3), x.data_ptr(), (img3 if s3 else img).data_ptr(), y.data_ptr(), None if affine else stat.data_ptr(),
                              scale.data_ptr() if affine else None, shift.data_ptr() if affine else None, relu, n, h, w, int(reflect), stream())
    assert rc == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    assert still_nan_fill(y[m:]), "the launch wrote behind the last output row"
    if stat is not None:
        assert still_nan_fill(stat[-GUARD:]), "the launch wrote behind the last statistics slot"
        stat = stat[:-GUARD]
    return y[:m], stat


@pytest.mark.parametrize("s3", [False, True], ids=["bf16", "split3"])
def test_stem_weight_image_of_nnf_has_the_documented_bits(s3):
    """nnf._stem_weights_fused builds the image stem_cases.stem_weight_image restates from vqseg.h: the tests below launch with the
    latter, the model with the former"""
    from vq_seg_amd import nnf
    _x, wt = sc.stem_operands("S1")
    got = nnf._stem_weights_fused(nn.Parameter(wt.to(dev())), s3)
    want = sc.stem_weight_image(wt, s3).reshape(64, -1)
    assert got.dtype == torch.int16 and tuple(got.shape) == tuple(want.shape)
    assert torch.equal(got.cpu(), want.view(torch.int16))


@pytest.mark.parametrize("case,reflect", STEM, ids=STEM_IDS)
def test_stem_raw_output_and_batchnorm_partials(case, reflect):
    """A.1 (s3 = 0, stat_partial, no scale): every element within dispatch_cases.bound(ref, S, 176) of the fp64 convolution of the
    bf16-rounded operands; the partials through vqseg_bn_finalize_f at the bars of _assert_batchnorm_statistics.  A.4: a second
    launch gives the same bits."""
    r = sc.stem_reference(case, reflect)
    y, stat = _stem(case, reflect)
    assert_inside(y, r["ref"], sc.stem_raw_bound(r), f"{case} raw")
    m = r["ref"].shape[0]
    filled = stat[:m // 64]                                      # 64 rows per slot; every strip is two whole slots
    assert bool(torch.isfinite(filled).all())
    _assert_batchnorm_statistics_of(r["ref"], stat)
    y2, stat2 = _stem(case, reflect)
    assert torch.equal(bits(y), bits(y2)) and torch.equal(bits(filled), bits(stat2[:m // 64]))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case,reflect", STEM, ids=STEM_IDS)
def test_stem_bf16_affine_epilogue(case, reflect, relu):
    """A.2: bf16(fma(acc, scale, shift)) [ReLU] against scale ref + shift in fp64 under stem_cases.stem_affine_bound"""
    r = sc.stem_reference(case, reflect)
    scale, shift = sc.stem_affine()
    pre, limit = sc.stem_affine_bound(r, scale, shift)
    y, _ = _stem(case, reflect, affine=True, relu=relu)
    assert_inside(y, torch.relu(pre) if relu else pre, limit, f"{case} affine relu={relu}")
    if relu:
        assert bool((y == 0).any()) and bool((y > 0).any()) and not bool((y < 0).any())


@pytest.mark.parametrize("case,reflect", STEM, ids=STEM_IDS)
def test_stem_split3_affine_epilogue(case, reflect):
    """A.3 (s3 = 1, rows [hi(64) | lo(64)], v = hi + lo): with ReLU (the model's launch) and without, under
    stem_cases.stem_s3_bound; hi is the nearest bf16 and lo a residual (|lo| <= 2^-8 |hi|); against the TRUE operation (fp64
    convolution of the unrounded fp32 operands) within 3e-5 of its maximum -- the bar test_nn_gpu holds this output to.  A.4: same
    bits from a second launch."""
    r = sc.stem_reference(case, reflect)
    scale, shift = sc.stem_affine()
    pre3, limit = sc.stem_s3_bound(r, scale, shift)
    for relu in (1, 0):
        y, _ = _stem(case, reflect, s3=True, affine=True, relu=relu)
        hi, lo = y[:, :64].double().cpu(), y[:, 64:].double().cpu()
        v = hi + lo
        assert_inside(v, torch.relu(pre3) if relu else pre3, limit, f"{case} split-3 relu={relu}")
        assert bool((lo.abs() <= 2.0 ** -8 * hi.abs()).all())
        true = scale.double() * r["true"] + shift.double()
        true = torch.relu(true) if relu else true
        err = ((v - true).abs().max() / true.abs().max()).item()
        print(f"{case} reflect={reflect} relu={relu}: split-3 against the true operation {err:.3e}")
        assert err <= 3e-5
        if relu:
            y2, _ = _stem(case, reflect, s3=True, affine=True, relu=1)
            assert torch.equal(bits(y), bits(y2))
            assert bool((v == 0).any()) and bool((v > 0).any())


def test_stem_entry_point_refuses_what_the_kernel_does_not_cover():
    """A.5: every call returns non-zero BEFORE any launch (vqseg_stem7_conv_f checks pointers, sizes, epilogue and alignment itself;
    launch_stem7_fused returns hipErrorInvalidValue for wo % 128 and for stem_fused = 0 before its launch) and leaves y and the
    statistics as they were."""
    L = lib()
    x = synth.uniform(1, (1, 8, 256, 3), -1, 1).to(dev())
    _x, wt = sc.stem_operands("S1")
    img, img3 = sc.stem_weight_image(wt, False).to(dev()), sc.stem_weight_image(wt, True).to(dev())
    scale, shift = (t.to(dev()) for t in sc.stem_affine())
    y = nan_rows(4 * 128 + GUARD, 128, BF16)
    stat = torch.full((16, 2, 64), float("nan"), dtype=F32, device=dev())
    X, I, I3, Y, ST, SC, SH = (t.data_ptr() for t in (x, img, img3, y, stat, scale, shift))
    calls = {
        "w = 250 (wo = 125)": (0, X, I, Y, ST, None, None, 0, 1, 8, 250, 0),
        "h = 3": (0, X, I, Y, ST, None, None, 0, 1, 3, 256, 1),
        "split-3 without scale": (1, X, I3, Y, ST, None, None, 0, 1, 8, 256, 0),
        "scale without shift": (0, X, I, Y, None, SC, None, 0, 1, 8, 256, 0),
        "null image": (0, None, I, Y, ST, None, None, 0, 1, 8, 256, 0),
        "null weights": (0, X, None, Y, ST, None, None, 0, 1, 8, 256, 0),
        "null output": (0, X, I, None, ST, None, None, 0, 1, 8, 256, 0),
        "output off by 2 bytes": (0, X, I, Y + 2, ST, None, None, 0, 1, 8, 256, 0),
    }
    for what, args in calls.items():
        assert L.vqseg_stem7_conv_f(*args, stream()) != 0, what
        assert L.vqseg_last_error(), what
    with option("stem_fused", 0):
        assert L.vqseg_stem7_conv_f(0, X, I, Y, ST, None, None, 0, 1, 8, 256, 0, stream()) != 0
        assert L.vqseg_stem7_conv_f(1, X, I3, Y, None, SC, SH, 1, 1, 8, 256, 1, stream()) != 0
    torch.cuda.synchronize()
    assert still_nan_fill(y) and still_nan_fill(stat)
    assert L.vqseg_stem7_conv_f(0, X, I, Y, ST, None, None, 0, 1, 8, 256, 0, stream()) == 0, "the option was not restored"
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.reshape(-1)[:512 * 64]).all())          # [512][64] rows at the head of the buffer


# ---------------------------------------------------------------------------------------------------------------------------
# B. vqseg_im2col_f.  The kernels report no variant id: the branch of launch_im2col_stem (nn_stem.hip) each case takes is
# read off its conditions and written next to the case.
# ---------------------------------------------------------------------------------------------------------------------------
STEM_GEOM = (3, 7, 2, 3)                                        # cin, k, stride, pad
IM2COL_STRIP_SHAPES = [
    (1, 4, 4),                  # wo = 2: one strip with 2 of its 64 / 128 pixels, the reflections of both borders in one strip
    (2, 5, 129),                # wo = 65: one pixel past a 64-pixel strip (fp32, split-3), inside the bf16 kernel's 128
    (1, 4, 257),                # wo = 129: one pixel past the bf16 kernel's 128-pixel strip
    (1, 9, 255),                # wo = 128: whole strips, odd width
]
IM2COL = []
for _shape in IM2COL_STRIP_SHAPES:
    for _reflect in (False, True):
        # branch 1 (im2col_stem7_strip_kernel): im2col_strip = 1, 7x7x3 / stride 2 / pad 3, kp = 160 (any form) or 192 (form 2):
        # <float, 64, 160>, <__bf16, 128, 160>, <S3Out, 64, 160>, <S3Out, 64, 192>
        IM2COL += [("strip", _shape, STEM_GEOM, _reflect, 160, f, 1) for f in (0, 1, 2)] + [("strip", _shape, STEM_GEOM, _reflect, 192, 2, 1)]
        # branch 2 (im2col_stem7_kernel<float / __bf16 / S3Out>): the same calls with im2col_strip = 0 fall through to the gather kernel
        IM2COL += [("gather", _shape, STEM_GEOM, _reflect, 160, f, 0) for f in (0, 1, 2)] + [("gather", _shape, STEM_GEOM, _reflect, 192, 2, 0)]
for _f in (0, 1, 2):
    for _reflect in (False, True):
        # branch 2 with the option ON: the strip launcher declines kp = 152 (neither 160 nor 192) ...
        IM2COL.append(("gather-kp152", (2, 5, 9), STEM_GEOM, _reflect, 152, _f, 1))
        # ... and stride 1 (its strips assume stride 2); 7x7x3 with kp % 8 == 0: the gather kernel
        IM2COL.append(("gather-s1p3", (1, 5, 6), (3, 7, 1, 3), _reflect, 160, _f, 1))
    # ... and pad 0 (no padding: reflect is not defined); 9 x 12 -> 2 x 3 output pixels
    IM2COL.append(("gather-s2p0", (1, 9, 12), (3, 7, 2, 0), False, 160, _f, 1))
for _f in (0, 1):
    for _reflect in (False, True):
        # branch 3 (im2col_stem_kernel<float, float / __bf16>): not 7x7x3 -> neither stem kernel
        IM2COL.append(("generic-3x3c4", (2, 5, 6), (4, 3, 1, 1), _reflect, 40, _f, 1))
        IM2COL.append(("generic-5x5c3", (1, 7, 9), (3, 5, 2, 2), _reflect, 80, _f, 1))
        # 7x7x3 but kp = 150: not the strip launcher's width, and kp % 8 != 0 rules out the gather kernel's 8-column stores
        IM2COL.append(("generic-kp150", (1, 6, 7), STEM_GEOM, _reflect, 150, _f, 1))


def _im2col_id(c):
    name, shape, geom, reflect, kp, form, strip = c
    return f"{name}-{'x'.join(map(str, shape))}-{'reflect' if reflect else 'zero'}-kp{kp}-form{form}"


_IMAGES = {}


def _image(shape, cin):
    if (shape, cin) not in _IMAGES:
        _IMAGES[(shape, cin)] = synth.uniform(sum(shape) + cin, (*shape, cin), -2.2, 2.7)
    return _IMAGES[(shape, cin)]


@pytest.mark.parametrize("c", IM2COL, ids=[_im2col_id(c) for c in IM2COL])
def test_im2col_equals_unfold_bit_for_bit(c):
    """form 0: F.unfold of the padded fp32 image, columns (kh, kw, ci), zero-extended to kp; form 1: its bf16 rounding; form 2:
    [hi | lo] with hi = bf16(v), lo = bf16(v - hi).  An exact operation: every bit, the zero columns included; guard rows keep NaN."""
    L = lib()
    _name, shape, (cin, k, stride, pad), reflect, kp, form, strip = c
    n, h, w = shape
    ho, wo = sc.im2col_out_size(h, w, k, stride, pad)
    m = n * ho * wo
    x = _image(shape, cin)
    want = sc.im2col_reference(x, k, stride, pad, reflect, kp, form)
    assert want.shape == (m, kp * (2 if form == 2 else 1))
    xd = x.to(dev())
    out = nan_rows(m + GUARD, want.shape[1], F32 if form == 0 else BF16)
    with option("im2col_strip", strip):
        rc = L.vqseg_im2col_f(form, xd.data_ptr(), n, h, w, cin, k, k, stride, pad, int(reflect), ho, wo, kp, out.data_ptr(), stream())
    assert rc == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    assert still_nan_fill(out[m:]), "the launch wrote behind the last patch row"
    got = out[:m].cpu()
    if not torch.equal(bits(got), bits(want)):
        r, col = (bits(got) != bits(want)).nonzero()[0].tolist()
        raise AssertionError(f"{int((bits(got) != bits(want)).sum())} elements differ, first at (row {r}, column {col}): "
                             f"got {float(got[r, col])!r}, want {float(want[r, col])!r}")
    kk = k * k * cin
    for part in ((got,) if form < 2 else (got[:, :kp], got[:, kp:])):
        assert not part[:, kk:].any()


def test_im2col_refusals_leave_the_output_untouched():
    """split-3 rows exist for the 7x7x3 stem only; reflect padding needs pad < h, w (one reflection, as F.pad: with h <= pad the
    kernels' guarded indices return something that is not reflect padding)"""
    L = lib()
    x = _image((1, 5, 6), 4).to(dev())
    out = nan_rows(64, 2 * 160, BF16)
    assert L.vqseg_im2col_f(2, x.data_ptr(), 1, 5, 6, 4, 3, 3, 1, 1, 0, 5, 6, 40, out.data_ptr(), stream()) != 0
    x3 = _image((1, 3, 8), 3).to(dev())
    for form in (0, 1, 2):
        for strip in (1, 0):
            with option("im2col_strip", strip):
                assert L.vqseg_im2col_f(form, x3.data_ptr(), 1, 3, 8, 3, 7, 7, 2, 3, 1, 2, 4, 160, out.data_ptr(), stream()) != 0
            assert b"reflect" in L.vqseg_last_error()
    assert L.vqseg_im2col_f(0, x3.data_ptr(), 1, 8, 3, 3, 7, 7, 2, 3, 1, 4, 2, 160, out.data_ptr(), stream()) != 0      # w <= pad
    torch.cuda.synchronize()
    assert still_nan_fill(out)
    # zero padding at the same size is defined and stays accepted
    outf = nan_rows(8 + GUARD, 160, F32)
    assert L.vqseg_im2col_f(0, x3.data_ptr(), 1, 3, 8, 3, 7, 7, 2, 3, 0, 2, 4, 160, outf.data_ptr(), stream()) == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    assert torch.equal(outf[:8].cpu(), sc.im2col_reference(_image((1, 3, 8), 3), 7, 2, 3, False, 160, 0)) and still_nan_fill(outf[8:])


# ---------------------------------------------------------------------------------------------------------------------------
# C. vqseg_reflect_fold_f
# ---------------------------------------------------------------------------------------------------------------------------
def _fold(case, bf16):
    L = lib()
    n, h, w, c = case
    gp = sc.fold_reference(case, bf16)[0]
    gpd = gp.to(dev())
    gx = nan_rows(n * h * w + GUARD, c, BF16 if bf16 else F32)
    rc = L.vqseg_reflect_fold_f(int(bf16), gpd.data_ptr(), n, h, w, c, gx.data_ptr(), stream())
    assert rc == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    assert still_nan_fill(gx[n * h * w:]), "the launch wrote behind the last pixel"
    return gx[:n * h * w].reshape(n, h, w, c)


def _check_fold(case, bf16, got):
    gp, ref, S, t = sc.fold_reference(case, bf16)
    one = t == 1
    assert torch.equal(bits(got.cpu()[one]), bits(gp[:, 1:-1, 1:-1][one])), "a pixel with one term is a copy"
    # t - 1 additions in fp32 (the first term meets an exact zero), then the store
    check(got, ref, S, t - 1, BF16 if bf16 else F32, f"reflect_fold {case} {'bf16' if bf16 else 'fp32'}")
    return t


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", sc.FOLD_CASES, ids=["x".join(map(str, c)) for c in sc.FOLD_CASES])
def test_reflect_fold_against_the_autograd_of_reflect_padding(case, bf16):
    """<__bf16, 8> (c % 8 == 0) / <__bf16, 1>, <float, 4> (c % 4 == 0) / <float, 1>: which padded positions fold onto which pixel"""
    n, h, w, c = case
    t = _check_fold(case, bf16, _fold(case, bf16))
    assert int(t.max()) == (3 if h == 3 else 2) * (3 if w == 3 else 2)           # rows x columns that reflect onto one pixel


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_reflect_fold_grid_stride_loop(bf16):
    """More work items than 256 x 256 threads under nn_grid_cap = 256 (the option's minimum): the second trip through the
    grid-stride loop gives the bits of the uncapped launch, and both meet the bound."""
    case = sc.FOLD_WRAP_CASE
    n, h, w, c = case
    assert n * h * w * (c // 8) > 256 * 256
    a = _fold(case, bf16)
    with option("nn_grid_cap", 256):
        b = _fold(case, bf16)
    assert torch.equal(bits(a), bits(b))
    _check_fold(case, bf16, b)


def test_reflect_fold_refuses_a_single_row():
    L = lib()
    gp = torch.zeros(1, 3, 6, 8, device=dev())
    gx = nan_rows(4 + GUARD, 8, F32)
    assert L.vqseg_reflect_fold_f(0, gp.data_ptr(), 1, 1, 4, 8, gx.data_ptr(), stream()) != 0
    assert L.vqseg_reflect_fold_f(0, gp.data_ptr(), 1, 4, 1, 8, gx.data_ptr(), stream()) != 0
    torch.cuda.synchronize()
    assert still_nan_fill(gx)


# ---------------------------------------------------------------------------------------------------------------------------
# D. vqseg_reflect_ring_f
# ---------------------------------------------------------------------------------------------------------------------------
def _ring_weights(wt, cgy, cgx):
    """the transposed, tap-flipped image of w [cgy, cgx, 3, 3]"""
    L = lib()
    t_hi = torch.empty(L.vqseg_conv_packed_elems(cgy, cgx, 3, 3, 1), dtype=torch.int16, device=dev())
    wd = wt.to(dev())
    assert L.vqseg_conv_pack_weights_f32(wd.data_ptr(), cgy, cgx, 3, 3, 1, t_hi.data_ptr(), None, stream()) == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    return t_hi


@pytest.mark.parametrize("case", sorted(sc.RING_CASES))
def test_reflect_ring_values_fold_and_variant(case):
    """D.1 the ring buffer equals the border of the fp64 padded gradient within dispatch_cases.bound(ref, S, 9 cgy); D.2 gx = G0 + the
    ring positions that reflect onto each pixel, summed in fp64 from the ring values READ BACK (the fold alone: G0 is arbitrary):
    untouched pixels keep G0's bits, the others meet check(k = added terms, bf16); D.3 the launch took the instantiation the ring
    branch of launch_conv_impl names for this cgx."""
    L = lib()
    n, h, w, cgy, cgx, want_id = sc.RING_CASES[case]
    gy, wt, g0 = sc.ring_operands(case)
    rl = sc.ring_len(h, w)
    t_hi = _ring_weights(wt, cgy, cgx)
    gyd = gy.to(dev())
    ring = nan_rows(n * rl + GUARD, cgx, BF16)
    gx = nan_rows(n * h * w + GUARD, cgx, BF16)
    gx[:n * h * w] = g0.reshape(-1, cgx).to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_reflect_ring_f(gyd.data_ptr(), t_hi.data_ptr(), ring.data_ptr(), gx.data_ptr(), n, h, w, cgy, cgx, stream())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == want_id, f"{case}: dispatched {got_id:#x}, the case is meant for {want_id:#x}"
    assert still_nan_fill(ring[n * rl:]) and still_nan_fill(gx[n * h * w:]), "the launch wrote behind a buffer"
    # D.1
    ref, S = sc.ring_reference(case)
    rv = ring[:n * rl].reshape(n, rl, cgx).cpu()
    assert_inside(rv, ref, sc.bound(ref, S, 9 * cgy), f"{case} ring")
    # D.2
    want, S2, k = sc.ring_fold_reference(g0, rv, h, w)
    got = gx[:n * h * w].reshape(n, h, w, cgx).cpu()
    touched = torch.zeros(h, w, dtype=torch.bool)
    touched[[1, h - 2], :] = True
    touched[:, [1, w - 2]] = True
    assert torch.equal(k[0, :, :, 0] > 0, touched) and int(k.max()) == 3
    assert torch.equal(bits(got[:, ~touched]), bits(g0[:, ~touched])), "a pixel off rows 1 / h-2 and columns 1 / w-2 changed"
    check(got, want, S2, k, BF16, f"{case} ring fold")


def test_reflect_ring_refusals_leave_the_buffers_untouched():
    L = lib()
    gy = torch.zeros(1 * 4 * 4 * 128, dtype=BF16, device=dev())
    t_hi = torch.zeros(L.vqseg_conv_packed_elems(128, 16, 3, 3, 1), dtype=torch.int16, device=dev())
    ring = nan_rows(sc.ring_len(4, 4) + GUARD, 16, BF16)
    gx = nan_rows(16 + GUARD, 16, BF16)
    for what, (h, cgy, cgx) in {"h = 3": (3, 64, 8), "cgy = 96": (4, 96, 8), "cgx = 12": (4, 64, 12)}.items():
        assert L.vqseg_reflect_ring_f(gy.data_ptr(), t_hi.data_ptr(), ring.data_ptr(), gx.data_ptr(), 1, h, 4, cgy, cgx, stream()) != 0, what
    torch.cuda.synchronize()
    assert still_nan_fill(ring) and still_nan_fill(gx)
