"""Elementwise fp64 parity of the fp32 ("precise", split-bf16) convolution kernels through the C ABI:
conv_igemm_kernel<128 | 64 | 32, true, 32> as forward convolution (raw output + BatchNorm partials, fused affine epilogue), stride-1
data gradient (transposed, tap-flipped image; reflect: on the padded grid, then vqseg_reflect_fold_f), stride-2 data gradient (parity
classes: vqseg_conv2d_dgrad_s2_f; dilated grid: up = 2) and conv_wgrad_kernel<TM, TN, true>, the per-tap weight gradient -- plus their
fast-mode siblings <.., false, 32> / <TM, TN, false> on bf16-exact operands.

Cases, operands, fp64 references and the bound (|y - ref| <= 2^-16 S + 3 K 2^-23 S + 2^-23 |ref|; no term from the kernels) are
tests/precise_cases.py's; tests/test_precise_bound_cpu.py shows without a GPU that the documented arithmetic meets the bound and that
dropped cross products, a dropped lo image, a clamped tail and a misplaced weight row do not.  Every launch is preceded by
`conv_last_variant = 0` and followed by an assertion on the id it reads back (conv_internal.h: conv_variant_igemm(bn, precise, 32,
false) = 0x20B01P0, conv_variant_wgrad_tap(tm, tn, precise) = 0x60MN0P0); outputs are pre-filled with NaN and followed by guard rows
that must keep their fill, workspaces by 0xA5 guard bytes.  Each check prints its worst error / bound before asserting (pytest -s)."""
import pytest
import torch
import torch.nn.functional as F

from tests import dispatch_cases as dc
from tests import precise_cases as pc
from tests import stem_cases
from tests import synth
from tests import test_dispatch_variants_gpu as tdv

pytestmark = pytest.mark.gpu

GUARD = 2                                                   # rows behind an output / slots behind the statistics
WS_GUARD = 4096                                             # bytes behind a weight-gradient workspace
U = pc.U

dev, _lib, _nan_fill = tdv.dev, tdv._lib, tdv._nan_like_fill


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _report(what, y, want, limit):
    """print the worst error / bound, then assert that no element is outside (NaN is; where the bound is 0 the value must be exact)"""
    y = y.double().cpu()
    err = (y - want).abs()
    pos = limit > 0
    ratio = float((err[pos] / limit[pos]).max()) if bool(pos.any()) else 0.0
    bad = (~(err <= limit)).nonzero()
    print(f"{what}: worst error / bound {ratio:.3g} ({int(pos.sum())} elements with a non-zero bound)")
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {y.numel()} elements outside the bound, first {i}: got {float(y[i])}, reference "
                             f"{float(want[i])}, bound {float(limit[i])}")
    return ratio


def _pack(wt, transpose_flip, lo):
    """vqseg_conv_pack_weights_f32 of wt [cout, cin, k, k] -> (hi, lo or None) on the GPU"""
    L = _lib()
    cout, cin, k, _ = wt.shape
    ne = L.vqseg_conv_packed_elems(cout, cin, k, k, transpose_flip)
    hi = torch.empty(ne, dtype=torch.int16, device=dev())
    lo_t = torch.empty(ne, dtype=torch.int16, device=dev()) if lo else None
    wd = wt.contiguous().to(dev())
    assert L.vqseg_conv_pack_weights_f32(wd.data_ptr(), cout, cin, k, k, transpose_flip, hi.data_ptr(), _ptr(lo_t), _st()) == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    return hi, lo_t


def _pack_s2(wt):
    L = _lib()
    cout, cin, k, _ = wt.shape
    ne = L.vqseg_conv_packed_s2_elems(cout, cin, k)
    hi = torch.empty(ne, dtype=torch.int16, device=dev())
    lo = torch.empty(ne, dtype=torch.int16, device=dev())
    wd = wt.contiguous().to(dev())
    assert L.vqseg_conv_pack_weights_s2_f32(wd.data_ptr(), cout, cin, k, hi.data_ptr(), lo.data_ptr(), _st()) == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    return hi, lo


def _conv(x, c1, hi, lo, geom, precise, want_id, stat=False, affine=None):
    """One vqseg_conv2d_f / vqseg_conv2d_affine_f launch over x [n, h, w, cin] (split at c1 into the two concat sources).
    geom = (cout, k, stride, pad, reflect, up, ho, wo); affine = (scale, shift, res with GUARD rows, relu) on the GPU.
    -> (y [m, cout], statistics slots or None); asserts the id and the guards."""
    L = _lib()
    n, h, w, cin = x.shape
    cout, k, stride, pad, reflect, up, ho, wo = geom
    m = n * ho * wo
    dt = torch.float32 if precise else torch.bfloat16
    xd = x.to(dt)
    x1 = xd[..., :c1].contiguous().to(dev())
    x2 = xd[..., c1:].contiguous().to(dev()) if c1 < cin else None
    y = torch.full((m + GUARD, cout), float("nan"), dtype=dt, device=dev())
    st_t = None
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    if affine is None:
        if stat:
            slots = L.vqseg_conv_stat_slots(m, cout)
            st_t = torch.full((slots + GUARD, 2, cout), float("nan"), dtype=torch.float32, device=dev())
        rc = L.vqseg_conv2d_f(x1.data_ptr(), _ptr(x2), c1, hi.data_ptr(), _ptr(lo), y.data_ptr(), _ptr(st_t), n, h, w, cin, cout, k, k, stride, pad,
                              int(reflect), up, ho, wo, int(precise), _st())
    else:
        scale, shift, res, relu = affine
        assert up == 1
        rc = L.vqseg_conv2d_affine_f(x1.data_ptr(), _ptr(x2), c1, hi.data_ptr(), _ptr(lo), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), int(relu),
                                     y.data_ptr(), n, h, w, cin, cout, k, k, stride, pad, int(reflect), ho, wo, int(precise), _st())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == want_id, f"dispatched {got_id:#x}, the case is meant for {want_id:#x}"
    assert _nan_fill(y[m:]), "the launch wrote behind the last output row"
    if st_t is not None:
        assert _nan_fill(st_t[-GUARD:]), "the launch wrote behind the last statistics slot"
        st_t = st_t[:-GUARD]
    return y[:m], st_t


def _forward(case, precise, **kw):
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    x, wt = pc.operands(case)
    hi, lo = _pack(wt, 0, precise)
    ho, wo = pc.out_size(case)
    return _conv(x, c1, hi, lo, (cout, k, stride, pad, reflect, 1, ho, wo), precise, pc.variant_of(case), **kw)


def _limit(case):
    ref, S = pc.reference(case)
    return pc.bound(ref, S, pc.contraction(case))


# ---------------------------------------------------------------------------------------------------------------------------
# a. forward: raw output + BatchNorm partials, the three BN tiles
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["F1", "F2", "F3", "F4", "F5", "F6"])
def test_precise_forward_raw_output_and_batchnorm_partials(case):
    """Ragged last tile (M % 128 != 0 in all six), Cout off the tile (20, 72, 136), Cin tails inside a stage (8, 20), concat splits
    inside and on a stage boundary, zero / reflect padding, stride 2 on odd sizes, three K stages per tap (F6): every output element
    within the bound; the partials through vqseg_bn_finalize_f at the bars of _assert_batchnorm_statistics_of; every slot of a
    pixel-row group that holds rows is finite."""
    y, stat = _forward(case, True, stat=True)
    ref, _S = pc.reference(case)
    _report(f"{case} forward", y, ref, _limit(case))
    m, cout = ref.shape
    rps = 64 if cout >= 64 else 32
    assert bool(torch.isfinite(stat[:(m + rps - 1) // rps]).all())
    tdv._assert_batchnorm_statistics_of(ref, stat)


# ---------------------------------------------------------------------------------------------------------------------------
# b. forward with the fused affine epilogue
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["F5", "F6", "F3"])
def test_precise_fused_affine_epilogue_with_residual_and_relu(case):
    """vqseg_conv2d_affine_f(precise = 1), one case per BN tile: y = relu(fma(acc, scale, shift) + res), all fp32.

    Against the fp64 t_ref = ref * scale + shift, y_ref = relu(t_ref + res):  |y - y_ref| <= B |scale| + 2^-22 (|t_ref| + |y_ref|)
    with B the convolution's bound.  The fma rounds once: |t - t_ref| <= B |scale| + 2^-24 |t|; the add rounds once: |s - s_ref| <=
    |t - t_ref| + 2^-24 |s| (s = t + res); |t| and |s| differ from |t_ref|, |s_ref| by terms already counted, which 2^-22 instead of
    2^-24 leaves room for (and B's additive term counts u = 2^-23 where round-to-nearest pays 2^-24: more than 2^-24 B).  ReLU does
    not increase a difference; where it clips the reference but not the result (s_ref < 0 < s), |y - y_ref| = s < |s - s_ref|, and
    the add's rounding there, at most 2^-24 |s| <= 2^-24 |s - s_ref|, is inside the same room: y_ref = 0 costs the bound nothing."""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    ref, S = pc.reference(case)
    m = ref.shape[0]
    sd = 900 + 10 * cout
    scale = synth.uniform(sd, (cout,), 0.5, 1.5) * torch.where(synth.uniform(sd + 1, (cout,)) < 0.3, -1.0, 1.0)
    shift = synth.uniform(sd + 2, (cout,), -2, 2)
    res = pc.full_mantissa(sd + 3, (m, cout)) * 4
    t_ref = ref * scale.double() + shift.double()
    y_ref = torch.relu(t_ref + res.double())
    limit = _limit(case) * scale.double().abs() + 2.0 ** -22 * (t_ref.abs() + y_ref.abs())
    res_d = torch.cat([res, torch.zeros(GUARD, cout)]).to(dev())
    y, _ = _forward(case, True, affine=(scale.to(dev()), shift.to(dev()), res_d, True))
    _report(f"{case} affine + residual + ReLU", y, y_ref, limit)
    assert bool((y == 0).any()) and bool((y > 0).any())      # the ReLU clipped something and passed something


# ---------------------------------------------------------------------------------------------------------------------------
# c. / d. data gradients
# ---------------------------------------------------------------------------------------------------------------------------
def _dgrad_generic(case, up):
    """the data gradient as vqseg_conv2d_f over gy with the transposed, tap-flipped image: [grid pixels, cin]"""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    gy, wt = pc.operands(case)
    hi, lo = _pack(wt, 1, True)
    gh, gw, gpad = pc.grad_grid(case)
    y, _ = _conv(gy, cout, hi, lo, (c1, k, 1, gpad, False, up, gh, gw), True, pc.variant_of(case))
    return y


def _fold(case, gp):
    """vqseg_reflect_fold_f (fp32) of gp [n (h + 2) (w + 2), c] on the GPU -> [n h w, c]; NaN pre-fill, guard rows"""
    L = _lib()
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    gx = torch.full((n * h * w + GUARD, c1), float("nan"), dtype=torch.float32, device=dev())
    assert L.vqseg_reflect_fold_f(0, gp.contiguous().data_ptr(), n, h, w, c1, gx.data_ptr(), _st()) == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    assert _nan_fill(gx[n * h * w:])
    return gx[:n * h * w]


def _fold_reference(case):
    """(fold of ref, its bound): the fold sums t padded positions per pixel (t = 1 inside, 2 on rows / columns 1 and h - 2 / w - 2, 4
    or more where they cross) in fp32, t - 1 roundings: on top of the fold of the convolution's bound, (t - 1) 2^-23 times the fold
    of what the terms can be in magnitude, |ref| + bound."""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    ref, _S = pc.reference(case)
    grid = lambda v: v.reshape(n, h + 2, w + 2, c1)
    b = _limit(case).expand_as(ref)
    t = stem_cases.reflect_fold(torch.ones(n, h + 2, w + 2, c1, dtype=torch.float64))
    folded = stem_cases.reflect_fold(grid(ref))
    limit = stem_cases.reflect_fold(grid(b)) + (t - 1) * U * stem_cases.reflect_fold(grid(ref.abs() + b))
    # the same gradient from autograd through the reflect padding itself
    gy, wt = pc.operands(case)
    x = torch.zeros(n, c1, h, w, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv2d(F.pad(x, (1,) * 4, mode="reflect"), wt.double(), stride=stride), x, gy.double().permute(0, 3, 1, 2))
    assert bool(((g.permute(0, 2, 3, 1) - folded).abs() <= 1e-12 * (1 + folded.abs())).all())
    return folded.reshape(-1, c1), limit.reshape(-1, c1)


def test_precise_stride1_data_gradient_with_zero_padding():
    """D1: the transpose_flip = 1 image, pad k - 1 - pad on the input grid; fp64 autograd gradient of F.conv2d (precise_cases checks
    its GEMM form against autograd on the CPU)"""
    y = _dgrad_generic("D1", 1)
    _report("D1 data gradient", y, pc.reference("D1")[0], _limit("D1"))
    assert bool(((pc.reference("D1")[0] - pc.autograd_reference("D1")).abs() <= 1e-13 * pc.reference("D1")[1]).all())


def test_precise_stride1_data_gradient_with_reflect_padding_and_fold():
    """D2: the full correlation on the padded 10 x 9 grid, then vqseg_reflect_fold_f; both stages within their bounds"""
    gp = _dgrad_generic("D2", 1)
    _report("D2 padded-grid gradient", gp, pc.reference("D2")[0], _limit("D2"))
    want, limit = _fold_reference("D2")
    _report("D2 folded gradient", _fold("D2", gp), want, limit)


def _dgrad_s2(case, accumulate=None):
    """vqseg_conv2d_dgrad_s2_f (precise) -> [grid pixels, cin]; accumulate: the tensor (CPU) the gradient is added to"""
    L = _lib()
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    gy, wt = pc.operands(case)
    hi, lo = _pack_s2(wt)
    gh, gw, _gpad = pc.grad_grid(case)
    ho, wo = pc.out_size(case)
    m = n * gh * gw
    gx = torch.full((m + GUARD, c1), float("nan"), dtype=torch.float32, device=dev())
    if accumulate is not None:
        gx[:m] = accumulate.to(dev())
    gyd = gy.to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_dgrad_s2_f(gyd.data_ptr(), hi.data_ptr(), lo.data_ptr(), gx.data_ptr(), n, ho, wo, cout, c1, k, gh, gw, 1,
                                   int(accumulate is not None), _st())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == pc.variant_of(case), hex(got_id)
    assert _nan_fill(gx[m:]), "the launch wrote behind the last gradient row"
    return gx[:m]


def _unfilled(case):
    """mask [grid pixels] of the pixels a 1x1 stride-2 gradient never reaches (odd row or column)"""
    _kind, n, h, w, *_rest = pc.CASES[case]
    odd = (torch.arange(h)[:, None] % 2 == 1) | (torch.arange(w)[None, :] % 2 == 1)
    return odd.repeat(n, 1, 1).reshape(-1)


@pytest.mark.parametrize("case", ["S1", "S2", "S3"])
def test_precise_stride2_data_gradient_parity_classes_and_dilated_grid(case):
    """vqseg_conv2d_dgrad_s2_f and vqseg_conv2d_f(up = 2) on the same operands, same reference, same bound (K = the parity class's taps
    x channels: the dilated launch's other taps meet exact zeros).  S1: k = 1 on odd h, w -- the pixels no gradient reaches are
    exactly 0 in both.  S2 / S3: k = 3 on the padded grid, odd / even sizes (elements with S = 0, such as the even case's last row
    and column, must be exactly 0: their bound is); S2 is then folded (reflect), S3 cropped (zero padding)."""
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, _acc = pc.CASES[case]
    ref, S = pc.reference(case)
    cls = _dgrad_s2(case)
    _report(f"{case} parity classes", cls, ref, _limit(case))
    dil = _dgrad_generic(case, 2)
    _report(f"{case} dilated grid", dil, ref, _limit(case))
    if k == 1:
        zero = _unfilled(case)
        assert bool((S[zero] == 0).all()) and bool((S[~zero] > 0).all())
        assert bool((cls[zero.to(dev())] == 0).all()) and bool((dil[zero.to(dev())] == 0).all())
    elif reflect:
        want, limit = _fold_reference(case)
        _report(f"{case} folded gradient", _fold(case, cls), want, limit)
    else:
        crop = lambda v: v.reshape(n, h + 2, w + 2, c1)[:, 1:-1, 1:-1].reshape(-1, c1)
        x = torch.zeros(n, c1, h, w, dtype=torch.float64, requires_grad=True)
        gy, wt = pc.operands(case)
        (g,) = torch.autograd.grad(F.conv2d(x, wt.double(), stride=2, padding=1), x, gy.double().permute(0, 3, 1, 2))
        want = g.permute(0, 2, 3, 1).reshape(-1, c1)
        assert bool(((want - crop(ref)).abs() <= 1e-13 * crop(S)).all())
        _report(f"{case} cropped gradient", crop(cls.cpu()), want, crop(_limit(case).expand_as(ref)))


def test_precise_stride2_1x1_data_gradient_accumulates_within_the_bound():
    """S1 with accumulate = 1 against other + gradient: the conv bound plus 2^-23 |other + ref| for the one fp32 add; pixels the
    gradient does not reach keep `other` bit for bit.  (Bit-identity with a separate add: test_optim_gpu.)"""
    case = "S1"
    ref, S = pc.reference(case)
    other = pc.full_mantissa(4242, tuple(ref.shape))
    acc = _dgrad_s2(case, accumulate=other)
    total = other.double() + ref
    _report("S1 accumulate", acc, total, pc.bound(ref, S, pc.contraction(case), total))
    zero = _unfilled(case)
    assert torch.equal(acc.cpu()[zero], other[zero])


# ---------------------------------------------------------------------------------------------------------------------------
# e. weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def _wgrad(case, precise, two_uses=False):
    """vqseg_conv2d_wgrad_f (two_uses: vqseg_conv2d_wgrad2_f over the batch cut into its first image and the rest) -> gw in the
    reference's layout [cout, (tap, ci)]"""
    L = _lib()
    _kind, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = pc.CASES[case]
    cin = c1 + c2
    ho, wo = pc.out_size(case)
    x, gy, prev = pc.operands(case)
    dt = torch.float32 if precise else torch.bfloat16
    cut = [(0, 1), (1, n)] if two_uses else [(0, n), None]
    src = []
    for rng in cut:
        if rng is None:
            src.append((None, None, None, 0))
            continue
        xs, gs = x[rng[0]:rng[1]].to(dt), gy[rng[0]:rng[1]].to(dt)
        src.append((gs.contiguous().to(dev()), xs[..., :c1].contiguous().to(dev()), xs[..., c1:].contiguous().to(dev()) if c2 else None, rng[1] - rng[0]))
    nbytes = L.vqseg_conv2d_wgrad_workspace_bytes(n, h, w, cin, ho, wo, cout, k, k)
    ws = torch.empty(nbytes + WS_GUARD, dtype=torch.uint8, device=dev())
    ws[nbytes:] = 0xA5
    numel = cout * cin * k * k
    gw = torch.full((numel + 64,), float("nan"), dtype=torch.float32, device=dev())
    if acc:
        gw[:numel] = prev.reshape(-1).to(dev())
    (ga, xa, xa2, na), (gb, xb, xb2, nb) = src
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_wgrad2_f(_ptr(ga), _ptr(xa), _ptr(xa2), na, _ptr(gb), _ptr(xb), _ptr(xb2), nb, c1, h, w, cin, ho, wo, cout, k, k, stride, pad,
                                 int(reflect), int(precise), cin, 0, int(acc), ws.data_ptr(), nbytes, gw.data_ptr(), _st()) if two_uses else \
        L.vqseg_conv2d_wgrad_f(_ptr(ga), _ptr(xa), _ptr(xa2), c1, n, h, w, cin, ho, wo, cout, k, k, stride, pad, int(reflect), int(precise), cin, 0,
                               int(acc), ws.data_ptr(), nbytes, gw.data_ptr(), _st())
    assert rc == 0, L.vqseg_last_error()
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == pc.variant_of(case), f"dispatched {got_id:#x}, the case is meant for {pc.variant_of(case):#x}"
    assert bool((ws[nbytes:] == 0xA5).all()), "the launch wrote behind its workspace"
    assert _nan_fill(gw[numel:]), "the launch wrote behind the gradient"
    m = n * ho * wo
    slabs = nbytes // (numel * 4)
    assert slabs * numel * 4 == nbytes and slabs == min((m + 255) // 256, 256), "the per-tap plan: at least 256 pixels per slab"
    return pc.to_rows(case, gw[:numel].reshape(cout, cin, k, k)), slabs


@pytest.mark.parametrize("case", ["W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "W9"])
def test_precise_weight_gradient(case):
    """conv_wgrad_kernel<TM, TN, true>, the six (TM, TN) pairs (Cout 136 / 72 / 40 x Cin 128 / 24): 3x3 zero and reflect, 1x1, stride 2,
    a concat split inside a 32-channel tile, M = 70 / 126 (ragged last stage) and 288 (two slabs), accumulate = 1 onto a full-mantissa
    gradient; gw pre-filled with NaN otherwise.  K = M + ceil(M / 32)."""
    ref, S = pc.reference(case)
    gw, slabs = _wgrad(case, True)
    assert slabs == (2 if case in ("W8", "W9") else 1)
    prev = pc.prev_rows(case)
    total = None if prev is None else prev.double() + ref
    _report(f"{case} weight gradient ({slabs} slab{'s' * (slabs > 1)})", gw, ref if prev is None else total, pc.bound(ref, S, pc.contraction(case), total))


def test_precise_weight_gradient_over_two_uses_in_one_launch():
    """W8 as vqseg_conv2d_wgrad2_f over its two images as two uses of the layer: same virtual batch, same reference, same bound"""
    ref, S = pc.reference("W8")
    gw, slabs = _wgrad("W8", True, two_uses=True)
    assert slabs == 2
    _report("W8 two uses", gw, ref, _limit("W8"))


# ---------------------------------------------------------------------------------------------------------------------------
# f. the fast-mode siblings: bf16-exact operands, products exact in fp32, only the accumulation (and the bf16 output) rounds
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["G1", "G2", "G3"])
def test_fast_register_staged_forward_with_cin_off_the_64_channel_chunk(case):
    """conv_igemm_kernel<128 | 64 | 32, false, 32> (Cin = 24, 40, 40 + 56): held to dispatch_cases.bound, 2^-8 |ref| + K 2^-23 S"""
    y, stat = _forward(case, False, stat=True)
    ref, S = pc.reference(case)
    _report(f"{case} bf16 forward", y, ref, dc.bound(ref, S, pc.contraction(case)))
    tdv._assert_batchnorm_statistics_of(ref, stat)


@pytest.mark.parametrize("case", ["V1", "V2", "V3", "V4", "V5", "V6"])
def test_fast_per_tap_weight_gradient_on_shapes_the_lds_dma_plans_refuse(case):
    """conv_wgrad_kernel<TM, TN, false> (Cout % 32 != 0, Wo % 16 != 0, Cin % 32 != 0 in V2 / V4 / V6): fp32 output of exact products,
    K 2^-23 S + 2^-23 |ref| with K = M + ceil(M / 32)"""
    ref, S = pc.reference(case)
    gw, slabs = _wgrad(case, False)
    _report(f"{case} bf16 weight gradient ({slabs} slab{'s' * (slabs > 1)})", gw, ref, pc.contraction(case) * U * S + U * ref.abs())
