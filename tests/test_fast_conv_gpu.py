"""Elementwise fp64 parity of the bf16 convolution kernels the training step spends its time in, through the C ABI:
  A  conv3x3_patch_kernel, every instantiation launch_conv3x3_patch takes without split-3, raw output + BatchNorm partials
  B  ... with the fused epilogues (vqseg_conv2d_affine_f: scale, shift, bf16 residual, ReLU; vqseg_conv2d_affine_bits_f: bit-masked
     addend) and in its data-gradient form (transposed, tap-flipped image)
  C  the 128-row conv_igemm_glds_kernel tiles with taps: 3x3 stride 1 on ragged sizes, 3x3 stride 2, 1x1 stride 2, one dilated launch
  D  the bf16 stride-2 data gradients: vqseg_conv2d_dgrad_s2_f on parity classes (k = 3, k = 1, accumulate) and
     vqseg_conv2d_dgrad_s2_fold_f (the three CLS instantiations + reflect_s2_ring_add_kernel)

Cases, bf16-exact operands, fp64 references, ids and bounds are tests/fast_cases.py's: dispatch_cases.bound, |y - ref| <= 2^-8 |ref| +
K 2^-23 S, on every element, and what the epilogues and the fold add to it by derivation (no term from a kernel).
tests/test_fast_bound_cpu.py shows without a GPU that the documented arithmetic meets these bounds and that a truncating store, a
dropped chunk, a zero halo column, a clamped last row and a fold without its corner do not.  Every launch is preceded by
`conv_last_variant = 0` and followed by an assertion on the id it reads back; outputs are pre-filled with NaN and followed by guard
rows that must keep their fill.  Each check prints its worst error / bound before asserting (pytest -s); profiles/fast_conv_parity.md
records them."""
import pytest
import torch

from tests import fast_cases as fc
from tests import synth
from tests import test_dispatch_variants_gpu as tdv
from tests import test_precise_conv_gpu as tpc

pytestmark = pytest.mark.gpu

GUARD = tpc.GUARD                                           # rows behind an output / an addend, slots behind the statistics
U = fc.U

dev, _lib, _nan_fill, _report, _st = tdv.dev, tdv._lib, tdv._nan_like_fill, tpc._report, tpc._st


def _geom(case):
    """(x or gy, c1, packed forward image, launch geometry of tpc._conv) of a forward case"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    x, wt = fc.operands(case)
    hi, _lo = tpc._pack(wt, 0, False)
    ho, wo = fc.out_size(case)
    return x, c1, hi, (cout, k, stride, pad, reflect, 1, ho, wo)


def _forward(case, want_id=None, more_options=None, **kw):
    """one launch of a forward case under its options (+ more_options): tpc._conv asserts the id and the guard rows"""
    x, c1, hi, geom = _geom(case)
    with tdv._Options({**fc.options(case), **(more_options or {})}):
        return tpc._conv(x, c1, hi, None, geom, False, fc.variant_of(case) if want_id is None else want_id, **kw)


def _assert_raw_output_and_statistics(case, y, stat):
    ref, _S = fc.reference(case)
    ratio = _report(f"{case} {fc.variant_of(case):#x} forward", y, ref, fc.limit(case))
    m, cout = ref.shape
    rps = 64 if cout >= 64 else 32
    assert bool(torch.isfinite(stat[:(m + rps - 1) // rps]).all())
    tdv._assert_batchnorm_statistics_of(ref, stat)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# A. the patch kernel, raw output + BatchNorm partials
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.A_CASES)
def test_patch_kernel_raw_output_and_batchnorm_partials(case):
    """Fourteen instantiations (fast_cases.A_IDS) at 16 x 64 .. 64 x 48 images: two tiles along each axis of the 8 x 32, 16 x 16,
    16 x 32 and 32 x 16 geometries, n = 2 (a halo row meets the next image), zero and reflect padding, concat splits on a 64- and a
    32-channel boundary, three Cout chunks.  Every output element within the bound, the partials at _patch_case's bars.  Several
    Cout chunks: the same launch on the 1-D XCD-pair grid reads back id | 1 and gives the same bits."""
    y, stat = _forward(case, stat=True)
    _assert_raw_output_and_statistics(case, y, stat)
    vid = fc.variant_of(case)
    if fc.geometry(case)[6] > 32 * (vid >> 16 & 15):
        y1, stat1 = _forward(case, vid | 1, {"conv3x3_patch_xcd_pair": 1}, stat=True)
        assert tdv._same_bits(y, y1) and tdv._same_bits(stat, stat1)


# ---------------------------------------------------------------------------------------------------------------------------
# B. the patch kernel's fused epilogues and its data-gradient form
# ---------------------------------------------------------------------------------------------------------------------------
def _epilogue_args(case):
    """(scale, shift, addend with GUARD rows of its own, bit field with guard bytes) on the GPU"""
    scale, shift, res, keep = fc.epilogue_operands(case)
    res_d = torch.cat([res.bfloat16(), torch.zeros(GUARD, res.shape[1], dtype=torch.bfloat16)]).to(dev())
    bits = torch.cat([fc.pack_bits(keep), torch.zeros(64, dtype=torch.uint8)]).to(dev())
    return scale.to(dev()), shift.to(dev()), res_d, bits


def _conv_bits(x, hi, geom, want_id, args):
    """one vqseg_conv2d_affine_bits_f launch over x [n, h, w, cin] (one source, zero padding); geom = (cout, k, pad, ho, wo)"""
    L = _lib()
    n, h, w, cin = x.shape
    cout, k, pad, ho, wo = geom
    m = n * ho * wo
    scale, shift, res, bits = args
    xd = x.bfloat16().contiguous().to(dev())
    y = torch.full((m + GUARD, cout), float("nan"), dtype=torch.bfloat16, device=dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_affine_bits_f(xd.data_ptr(), hi.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), bits.data_ptr(), y.data_ptr(),
                                      n, h, w, cin, cout, k, k, pad, ho, wo, _st())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == want_id, f"dispatched {got_id:#x}, the case is meant for {want_id:#x}"
    assert _nan_fill(y[m:]), "the launch wrote behind the last output row"
    return y[:m]


@pytest.mark.parametrize("form", ["affine", "bits"])
@pytest.mark.parametrize("case", fc.EPILOGUE_CASES)
def test_patch_kernel_fused_affine_epilogues(case, form):
    """vqseg_conv2d_affine_f (scale, shift, bf16 residual, ReLU) and vqseg_conv2d_affine_bits_f (bit-masked addend) on 0x3143210 with
    three chunks, 0x3182200, 0x3123210, a chunk-stage and a 512-pixel instantiation: the 2-D TileRows row map feeds the residual
    read, the bit read, the ReLU and the write-out.  Bound: fast_cases.epilogue_reference, 2^-8 |y_ref| + 2^-8 |t_ref| +
    K 2^-23 S |scale|."""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    assert c2 == 0 and not reflect
    y_ref, limit = fc.epilogue_reference(case, form)
    args = _epilogue_args(case)
    if form == "affine":
        y, _ = _forward(case, affine=(args[0], args[1], args[2], True))
        assert bool((y == 0).any()) and bool((y > 0).any())      # the ReLU clipped something and passed something
    else:
        x, _c1, hi, _g = _geom(case)
        with tdv._Options(fc.options(case)):
            y = _conv_bits(x, hi, (cout, k, pad, h, w), fc.variant_of(case), args)
    _report(f"{case} {fc.variant_of(case):#x} {form}", y, y_ref, limit)


def test_patch_kernel_data_gradient_form_of_a_concat_layer():
    """G1: the gradient of a 64 + 64 -> 256 layer for all 128 input channels in one launch, vqseg_conv_pack_weights_f32(..,
    transpose_flip = 1) with Cin and Cout swapped, id 0x3143210: through vqseg_conv2d_f against the GEMM-form reference (which agrees
    with fp64 autograd to 1e-13 S), and through vqseg_conv2d_affine_bits_f with real scales and shifts (the masked shortcut add of
    backward)."""
    case = "G1"
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    cin = c1 + c2
    gy, wt = fc.operands(case)
    ref, S = fc.reference(case)
    assert bool(((ref - fc.autograd_gradient(case)).abs() <= 1e-13 * S).all())
    thi, _lo = tpc._pack(wt, 1, False)
    with tdv._Options(fc.options(case)):
        gx, _ = tpc._conv(gy, cout, thi, None, (cin, k, 1, k - 1 - pad, False, 1, h, w), False, fc.variant_of(case))
        masked = _conv_bits(gy, thi, (cin, k, k - 1 - pad, h, w), fc.variant_of(case), _epilogue_args(case))
    _report(f"{case} data-gradient form", gx, ref, fc.limit(case))
    y_ref, limit = fc.epilogue_reference(case, "bits")
    _report(f"{case} data-gradient form, bit-masked addend", masked, y_ref, limit)


# ---------------------------------------------------------------------------------------------------------------------------
# C. the 128-row LDS-DMA tiles with taps
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fc.C_CASES)
def test_lds_dma_tiles_with_taps_and_strides(case):
    """Default options, shapes the patch kernel refuses, M % 128 != 0 in all of them: 3x3 stride 1 at 2 x 9 x 11 (64 -> 128, 128 -> 64
    reflect, 64 + 64 -> 32), 3x3 stride 2 on 17 x 15 (reflect 64 -> 64; zero 128 -> 256 on the XCD-pair grid), 1x1 stride 2 (128 ->
    192 with a half-filled second chunk on the single-buffer tile, 64 -> 128 with one K stage).  The generic prologue's pixel
    arithmetic, raw output + BatchNorm partials."""
    y, stat = _forward(case, stat=True)
    _assert_raw_output_and_statistics(case, y, stat)


def _dgrad_dilated(case):
    """the stride-2 data gradient as ONE vqseg_conv2d_f launch over the zero-dilated gy (up = 2) with the transposed, tap-flipped image"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    gy, wt = fc.operands(case)
    thi, _lo = tpc._pack(wt, 1, False)
    gh, gw, gpad = fc.grad_grid(case)
    y, _ = tpc._conv(gy, cout, thi, None, (c1, k, 1, gpad, False, 2, gh, gw), False, fc.glds_id(64, 3))
    return y


def test_lds_dma_tile_on_the_dilated_grid():
    """C4: S2 (the gradient of C2a's layer) as an up = 2 launch, nine K stages on <128, 64, 4, 3>: held to the parity class's K --
    the other taps meet exact zeros, and x + 0 rounds nothing"""
    _report("S2 dilated grid", _dgrad_dilated("S2"), fc.reference("S2")[0], fc.limit("S2"))


# ---------------------------------------------------------------------------------------------------------------------------
# D. stride-2 data gradients in bf16
# ---------------------------------------------------------------------------------------------------------------------------
def _dgrad_s2(case, accumulate=None):
    """vqseg_conv2d_dgrad_s2_f(precise = 0) -> [grid pixels, cin] bf16; accumulate: the bf16-exact tensor (CPU) the gradient is added to"""
    L = _lib()
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    gy, wt = fc.operands(case)
    hi, _lo = tpc._pack_s2(wt)
    gh, gw, _gpad = fc.grad_grid(case)
    ho, wo = fc.out_size(case)
    m = n * gh * gw
    gx = torch.full((m + GUARD, c1), float("nan"), dtype=torch.bfloat16, device=dev())
    if accumulate is not None:
        gx[:m] = accumulate.bfloat16().to(dev())
    gyd = gy.bfloat16().to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_dgrad_s2_f(gyd.data_ptr(), hi.data_ptr(), None, gx.data_ptr(), n, ho, wo, cout, c1, k, gh, gw, 0, int(accumulate is not None), _st())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == fc.variant_of(case), f"dispatched {got_id:#x}, the case is meant for {fc.variant_of(case):#x}"
    assert _nan_fill(gx[m:]), "the launch wrote behind the last gradient row"
    return gx[:m]


@pytest.mark.parametrize("case", fc.S2_K3_CASES)
def test_stride2_data_gradient_parity_classes_on_the_padded_grid(case):
    """k = 3 on the padded grid, `omap` placement of the four parity classes: odd input sizes (S2, S4) and even ones (S3, S5), gy with
    64 channels on the LDS-DMA tiles and with 40 on conv_igemm_kernel<.., false, 32>.  K per pixel is the parity class's count; the
    even cases' last row and column (S = 0) are exactly 0."""
    _kind, n, h, w, c1, *_rest = fc.geometry(case)
    ref, S = fc.reference(case)
    gx = _dgrad_s2(case)
    _report(f"{case} {fc.variant_of(case):#x} parity classes", gx, ref, fc.limit(case))
    if h % 2 == 0:
        g = gx.reshape(n, h + 2, w + 2, c1)
        assert bool((S.reshape(n, h + 2, w + 2, c1)[:, -1] == 0).all()) and bool((S.reshape(n, h + 2, w + 2, c1)[:, :, -1] == 0).all())
        assert bool((g[:, -1] == 0).all()) and bool((g[:, :, -1] == 0).all())


def _unreached(case):
    """mask [grid pixels] of the pixels a 1x1 stride-2 gradient never reaches (odd row or column)"""
    _kind, n, h, w, *_rest = fc.geometry(case)
    odd = (torch.arange(h)[:, None] % 2 == 1) | (torch.arange(w)[None, :] % 2 == 1)
    return odd.repeat(n, 1, 1).reshape(-1)


@pytest.mark.parametrize("case", fc.S2_K1_CASES)
def test_stride2_1x1_data_gradient_plain_and_accumulating(case):
    """k = 1 on odd sizes: pixels no gradient reaches are exactly 0.  accumulate = 1 onto a bf16 `other` (ep_res_out): the kernel
    rounds the gradient to bf16, adds `other` in fp32 and rounds again -- 2^-8 |other + ref| + 2^-8 |ref| + K 2^-23 S, the affine
    derivation with unit scale; unreached pixels keep `other` bit for bit."""
    ref, S = fc.reference(case)
    K = fc.contraction(case)
    zero = _unreached(case)
    assert bool((S[zero] == 0).all()) and bool((S[~zero] > 0).all())
    gx = _dgrad_s2(case)
    _report(f"{case} {fc.variant_of(case):#x} k = 1", gx, ref, fc.limit(case))
    assert bool((gx[zero.to(dev())] == 0).all())
    other = synth.uniform(4242, tuple(ref.shape), -1, 1).bfloat16()
    acc = _dgrad_s2(case, accumulate=other)
    total = other.double() + ref
    _report(f"{case} accumulate", acc, total, 2.0 ** -8 * total.abs() + 2.0 ** -8 * ref.abs() + K * U * S)
    assert tdv._same_bits(acc.cpu()[zero], other[zero])


@pytest.mark.parametrize("case", fc.FOLD_CASES)
def test_stride2_data_gradient_in_one_launch_with_the_ring_fold(case):
    """vqseg_conv2d_dgrad_s2_fold_f on the three CLS instantiations (0x1144142, 0x1144212, 0x1124312) + reflect_s2_ring_add_kernel:
    vqseg_conv2d_dgrad_s2_fold_rows(..) + GUARD rows, NaN-filled; the guard rows keep their fill, the first n h w rows are finite
    (ring region and dump row: unspecified).  Reference: fp64 autograd through the reflect / zero padding; bound:
    fast_cases.fold_reference (dispatch_cases.bound with the parity class's K; on x row 1 / column 1 of a reflect case the fold of
    the per-position bounds, the fp32 additions and the second rounding)."""
    L = _lib()
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    gy, wt = fc.operands(case)
    hi, _lo = tpc._pack_s2(wt)
    want, limit = fc.fold_reference(case)
    rows = int(L.vqseg_conv2d_dgrad_s2_fold_rows(n, h, w, int(reflect)))
    assert rows == n * h * w + (n * (w + 1 + h) if reflect else 0) + 1
    buf = torch.full((rows + GUARD, c1), float("nan"), dtype=torch.bfloat16, device=dev())
    gyd = gy.bfloat16().to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_dgrad_s2_fold_f(gyd.data_ptr(), hi.data_ptr(), buf.data_ptr(), n, h // 2, w // 2, cout, c1, h, w, int(reflect), _st())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == fc.variant_of(case), f"dispatched {got_id:#x}, the case is meant for {fc.variant_of(case):#x}"
    assert _nan_fill(buf[rows:]), "the launch wrote behind the rows vqseg_conv2d_dgrad_s2_fold_rows asks for"
    gx = buf[:n * h * w]
    assert bool(torch.isfinite(gx).all())
    _report(f"{case} {fc.variant_of(case):#x} merged fold", gx, want, limit)
    if reflect:
        t = fc.touched(case).repeat(n, 1, 1).reshape(-1)
        _report(f"{case} ... x row 1 / column 1 alone", gx[t.to(dev())], want[t], limit[t])
