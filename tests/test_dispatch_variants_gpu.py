"""GPU parity of the kernel instantiations that only full-size layers dispatch, at the smallest shapes that still reach them.

Convolutions go through the C ABI on bf16-exact operands against the fp64 reference of tests/dispatch_cases.py, elementwise at
its bound (|y - ref| <= 2^-8 |ref| + K 2^-23 S); outputs are pre-filled with NaN and followed by guard rows that must keep their
fill; BatchNorm partials go through vqseg_bn_finalize_f as nnf hands them over.  Every launch is preceded by
`conv_last_variant = 0` and followed by an assertion on the id it reads back (conv_internal.h: 0x1TBWUMf = pixel tile / 128, Cout
tile / 32, waves, buffers, min waves per SIMD, flags split-3 8 | linear-pixel prologue 4 | parity classes 2 | XCD-pair grid 1), so
a case that a retuned threshold moves to another instantiation fails instead of silently testing something else.

The VQ cases compare indices and winning-distance bits with the chain oracle at every tiles-per-wave count T, which
vqseg_vq_tiles_per_wave reports."""
import numpy as np
import pytest
import torch

from tests import dispatch_cases as dc
from tests import synth

pytestmark = pytest.mark.gpu

GUARD = 2                                                       # rows after the last output row / slots after the last statistics slot


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _lib():
    from vq_seg_amd import _hip
    return _hip.lib()


class _Options:
    """set the given options, restore them on exit"""

    def __init__(self, opts):
        self.opts, self.prev = opts, {}

    def __enter__(self):
        L = _lib()
        for k, v in self.opts.items():
            self.prev[k] = L.vqseg_set_option(k.encode(), v)
            assert self.prev[k] >= 0, L.vqseg_last_error()

    def __exit__(self, *exc):
        L = _lib()
        for k, v in self.prev.items():
            L.vqseg_set_option(k.encode(), v)


def _nan_like_fill(t):
    return torch.equal(t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32), torch.full_like(t, float("nan")).view(
        torch.int16 if t.dtype == torch.bfloat16 else torch.int32))


_DEVICE_OPERANDS = {}


def _device_operands(case):
    """(x, packed weights) of the case on the GPU, uploaded and packed once"""
    if case not in _DEVICE_OPERANDS:
        L = _lib()
        n, h, w, cin, cout, k, stride, pad, reflect = dc.CASES[case]
        x, wt = dc.operands(case)
        hi = torch.empty(L.vqseg_conv_packed_elems(cout, cin, k, k, 0), dtype=torch.int16, device=dev())
        wd = wt.to(dev())
        assert L.vqseg_conv_pack_weights_f32(wd.data_ptr(), cout, cin, k, k, 0, hi.data_ptr(), None, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        _DEVICE_OPERANDS[case] = (x.to(dev()), hi)
    return _DEVICE_OPERANDS[case]


def _conv(case, opts, want_id, epilogue="stat", affine=None):
    """One launch of the case under `opts`: (y [M, cout] bf16, statistics slots or None).  Asserts the variant id and that the guard
    rows behind y and behind the statistics kept their NaN fill.  epilogue: "stat" (raw y + BatchNorm partials, vqseg_conv2d_f),
    "affine" (scale / shift + residual + ReLU, vqseg_conv2d_affine_f) or "bits" (scale / shift + bit-masked addend,
    vqseg_conv2d_affine_bits_f); affine = (scale, shift, res, bits) on the GPU."""
    L = _lib()
    n, h, w, cin, cout, k, stride, pad, reflect = dc.CASES[case]
    ho, wo = dc.out_size(case)
    m = n * ho * wo
    x, hi = _device_operands(case)
    st = torch.cuda.current_stream().cuda_stream
    y = torch.full((m + GUARD, cout), float("nan"), dtype=torch.bfloat16, device=dev())
    stat = None
    with _Options(opts):
        assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
        if epilogue == "stat":
            slots = L.vqseg_conv_stat_slots(m, cout)
            stat = torch.full((slots + GUARD, 2, cout), float("nan"), dtype=torch.float32, device=dev())
            rc = L.vqseg_conv2d_f(x.data_ptr(), None, cin, hi.data_ptr(), None, y.data_ptr(), stat.data_ptr(), n, h, w, cin, cout, k, k,
                                  stride, pad, int(reflect), 1, ho, wo, 0, st)
        elif epilogue == "affine":
            scale, shift, res, _bits = affine
            rc = L.vqseg_conv2d_affine_f(x.data_ptr(), None, cin, hi.data_ptr(), None, scale.data_ptr(), shift.data_ptr(), res.data_ptr(), 1,
                                         y.data_ptr(), n, h, w, cin, cout, k, k, stride, pad, int(reflect), ho, wo, 0, st)
        else:
            scale, shift, res, bits = affine
            assert stride == 1
            rc = L.vqseg_conv2d_affine_bits_f(x.data_ptr(), hi.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), bits.data_ptr(),
                                              y.data_ptr(), n, h, w, cin, cout, k, k, pad, ho, wo, st)
        assert rc == 0, L.vqseg_last_error()
        got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got_id == want_id, f"{case} {opts}: dispatched {got_id:#x}, the case is meant for {want_id:#x}"
    assert _nan_like_fill(y[m:]), "the launch wrote behind the last output row"
    if stat is not None:
        assert _nan_like_fill(stat[-GUARD:]), "the launch wrote behind the last statistics slot"
        stat = stat[:-GUARD]
    return y[:m], stat


def _assert_within_bound(case, y, what):
    ref, S = dc.reference(case)
    bad = dc.violations(y.cpu(), ref, S, dc.contraction(case))
    if len(bad):
        r, c = bad[0].tolist()
        raise AssertionError(f"{case} {what}: {len(bad)} elements outside the bound, first (row {r}, channel {c}): got {float(y[r, c])}, "
                             f"reference {float(ref[r, c])}, bound {float(dc.bound(ref, S, dc.contraction(case))[r, c])}")


def _assert_batchnorm_statistics(case, stat):
    _assert_batchnorm_statistics_of(dc.reference(case)[0], stat)


def _assert_batchnorm_statistics_of(ref, stat):
    """the partials through vqseg_bn_finalize_f (training form, as nnf._bn_finalize) against the fp64 output ref [M, C]: mean within
    1e-5 of max |ref|, biased variance within 1e-4 of the largest variance -- the bars of test_nn_gpu._patch_case"""
    L = _lib()
    m, c = ref.shape
    eps, d = 1e-5, dev()
    part = stat.clone()                                         # finalize merges in place
    gamma, beta = torch.ones(c, device=d), torch.zeros(c, device=d)
    run_mean, run_var = torch.zeros(c, device=d), torch.ones(c, device=d)
    coef = torch.full((4, c), float("nan"), device=d)
    nbt = torch.zeros(1, dtype=torch.int64, device=d)
    rc = L.vqseg_bn_finalize_f(part.data_ptr(), m, c, gamma.data_ptr(), beta.data_ptr(), run_mean.data_ptr(), run_var.data_ptr(), 0.1, eps, 1,
                               coef[0].data_ptr(), coef[1].data_ptr(), coef[2].data_ptr(), coef[3].data_ptr(), nbt.data_ptr(), None,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.vqseg_last_error()
    torch.cuda.synchronize()
    mean = coef[2].double().cpu()
    var = coef[3].double().cpu() ** -2 - eps
    assert int(nbt) == 1
    assert ((mean - ref.mean(0)).abs().max() / ref.abs().max()).item() < 1e-5
    want_var = ref.var(0, unbiased=False)
    assert ((var - want_var).abs().max() / want_var.max()).item() < 1e-4


def _filled_slots(case, stat):
    ref, _S = dc.reference(case)
    m, c = ref.shape
    rps = 64 if c >= 64 else 32
    return stat[:(m + rps - 1) // rps]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# E1-E4: the eight-wave 256 x 128 tile, <256, 128, 8, 3>.  id 0x12483 1 f.
# ---------------------------------------------------------------------------------------------------------------------------
BIG_TILE = [
    # case, id on the 2-D grid, id on the XCD-pair grid, which of the two the default options take
    ("E1", 0x1248314, 0x1248315, 0),       # 1x1 s1: linear-pixel prologue; 16 chunks > conv_xcd_pair = 8: 2-D grid by default
    ("E2", 0x1248314, 0x1248315, 1),       # 8 chunks: pair grid by default, 67 M tiles -> 72 per chunk, five return early
    ("E3", 0x1248310, 0x1248311, 1),       # 3x3 stride 2 reflect, odd sizes: generic prologue; 65 tiles -> 72
    ("E4", 0x1248310, 0x1248311, 0),       # 1x1 stride 2 (projection shortcut): generic prologue
]


@pytest.mark.parametrize("case,id_2d,id_pair,default", BIG_TILE, ids=[c[0] for c in BIG_TILE])
def test_256x128_tile_raw_output_and_batchnorm_partials(case, id_2d, id_pair, default):
    """Ragged last tile (M % 256 != 0 in all four), both grids, the stat_partial epilogue: each grid's output within the bound,
    statistics at _patch_case's bars, and the two grids bit-identical (same workgroups, same accumulation order, other ids)."""
    y0, s0 = _conv(case, {"conv_xcd_pair": 0}, id_2d)
    y1, s1 = _conv(case, {"conv_xcd_pair": 16}, id_pair)
    yd, sd = _conv(case, {}, (id_2d, id_pair)[default])
    _assert_within_bound(case, y0, "2-D grid")
    _assert_batchnorm_statistics(case, s0)
    assert _same_bits(y0, y1) and _same_bits(y0, yd)
    f0 = _filled_slots(case, s0)
    assert bool(torch.isfinite(f0).all())
    assert _same_bits(f0, _filled_slots(case, s1)) and _same_bits(f0, _filled_slots(case, sd))


@pytest.mark.parametrize("epilogue", ["affine", "bits"])
def test_256x128_tile_fused_affine_epilogues_on_the_pair_grid(epilogue):
    """E2 through vqseg_conv2d_affine_f (scale, shift, residual, ReLU) and vqseg_conv2d_affine_bits_f (scale, shift, bit-masked
    addend): id 0x1248315 (pair grid, the default at 8 chunks; 67 tiles: padding workgroups return early) and 0x1248314.

    The kernel rounds t = acc * scale + shift to bf16, adds the bf16 addend in fp32 and rounds again, so against the fp64
    y_ref = [relu](t_ref + addend), t_ref = ref * scale + shift, the bound of dispatch_cases grows by the first rounding and scales its
    accumulation term: |y - y_ref| <= 2^-8 |y_ref| + 2^-8 |t_ref| + K 2^-23 S |scale| (each rounding is within 2^-9 of its
    argument, which differs from the fp64 one by the terms already counted; 2^-8 and u = 2^-23 leave room for that and for the two
    fp32 roundings of the fma and the add; ReLU does not increase a difference)."""
    case = "E2"
    ref, S = dc.reference(case)
    m, c = ref.shape
    K = dc.contraction(case)
    scale = synth.uniform(71, (c,), 0.5, 1.5)
    shift = synth.uniform(72, (c,), -0.5, 0.5)
    res = synth.uniform(73, (m, c), -1, 1).bfloat16()
    keep = synth.uniform(74, (m, c), -1, 1) > 0
    bits = (keep.reshape(-1, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)
    t_ref = ref * scale.double() + shift.double()
    if epilogue == "affine":
        y_ref = torch.relu(t_ref + res.double())
    else:
        y_ref = t_ref + torch.where(keep, res.double(), torch.zeros((), dtype=torch.float64))
    limit = 2.0 ** -8 * y_ref.abs() + 2.0 ** -8 * t_ref.abs() + K * 2.0 ** -23 * S * scale.double().abs()
    # (the addend buffer gets guard rows of its own so that a read behind it would not fault either way)
    res_d = torch.cat([res, torch.zeros(GUARD, c, dtype=torch.bfloat16)]).to(dev())
    args = (scale.to(dev()), shift.to(dev()), res_d, bits.to(dev()))
    y1, _ = _conv(case, {}, 0x1248315, epilogue, args)
    y0, _ = _conv(case, {"conv_xcd_pair": 0}, 0x1248314, epilogue, args)
    bad = (~((y1.double().cpu() - y_ref).abs() <= limit)).nonzero()
    assert len(bad) == 0, f"{len(bad)} elements outside the bound, first (row, channel) {bad[0].tolist()}"
    assert _same_bits(y0, y1)
    if epilogue == "affine":
        assert bool((y1 == 0).any()) and bool((y1 > 0).any())    # the ReLU clipped something and passed something


def test_256x128_tile_split3_through_nnf():
    """E5: E1's layer with 192 logical channels as a split-3 launch (fp32 values as [hi | lo] bf16 rows, contraction over
    3 x 192 = 576 channels = nine K stages) through nnf.conv_bn_act(nnf.to_s3(..)) with eval BatchNorm + ReLU: id 0x124831c (split-3,
    linear-pixel prologue, 2-D grid: 16 chunks); fp64 reference of the fp32 operands, 2e-5 of scale (test_s3_gpu's bar)."""
    from torch import nn
    from vq_seg_amd import nnf
    L = _lib()
    n, h, w, _cin, cout, k, stride, pad, reflect = dc.CASES["E1"]
    cin = 192
    torch.manual_seed(192 + cout)
    conv = nn.Conv2d(cin, cout, 1, bias=False)
    bn = nn.BatchNorm2d(cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5), bn.bias.uniform_(-0.5, 0.5), bn.running_mean.uniform_(-0.2, 0.2), bn.running_var.uniform_(0.5, 1.5)
    bn.eval()
    x = synth.relu_features(5, (n, cin, h, w))
    rows = x.double().permute(0, 2, 3, 1).reshape(-1, cin) @ conv.weight.detach().double().reshape(cout, cin).t()
    want = torch.relu((rows - bn.running_mean.double()) / torch.sqrt(bn.running_var.double() + bn.eps) * bn.weight.detach().double() + bn.bias.detach().double())
    conv, bn = conv.to(dev()), bn.to(dev())
    xs = nnf.to_s3(x.to(dev()).contiguous(memory_format=torch.channels_last))
    L.vqseg_set_option(b"conv_last_variant", 0)
    with torch.no_grad():
        got = nnf.conv_bn_act(xs, conv, bn, relu=True)
    got_id = L.vqseg_set_option(b"conv_last_variant", 0)
    assert got_id == 0x124831c, hex(got_id)
    assert isinstance(got, nnf.S3) and got.shape == (n, cout, h, w)
    y = got.float().permute(0, 2, 3, 1).reshape(-1, cout).double().cpu()
    err = (y - want).abs()
    r, c = divmod(int(err.argmax()), cout)
    assert (err.max() / want.abs().max()).item() < 2e-5, f"largest error at (row {r}, channel {c})"


# ---------------------------------------------------------------------------------------------------------------------------
# F1-F5: 1x1 layers at M = 333 on the 128-row tiles
# ---------------------------------------------------------------------------------------------------------------------------
SMALL_TILE = [
    # case, id with the linear-pixel prologue (default), id with conv_linear_prologue = 0
    ("F1", 0x1144215, 0x1144211),          # 1024 -> 256: <128, 128, 4, 2>, 16 K stages; 2 chunks: pair grid (3 M tiles -> 8 per chunk)
    ("F2", 0x1144215, 0x1144211),          # 2048 -> 512: 32 K stages, 4 chunks
    ("F3", 0x1144215, 0x1144211),          # 640 -> 192: the second chunk is half filled
    ("F4", 0x1114314, 0x1114310),          # 128 -> 32: <128, 32, 4, 3>, one chunk: 2-D grid
    ("F5", 0x1124314, 0x1124310),          # 128 -> 64: <128, 64, 4, 3>
]


@pytest.mark.parametrize("case,id_lin,id_generic", SMALL_TILE, ids=[c[0] for c in SMALL_TILE])
def test_deep_k_and_narrow_1x1_layers_with_both_prologues(case, id_lin, id_generic):
    """Deep K loops (16 / 32 stages through a two- or three-slot ring), a part-filled last chunk and the 32- / 64-wide tiles, each
    with the linear-pixel prologue and with the generic one: within the bound, statistics at _patch_case's bars, and -- the prologue
    only computes where a row's pixels start, the stages and their order are the same -- bit-identical output and partials."""
    y1, s1 = _conv(case, {}, id_lin)
    y0, s0 = _conv(case, {"conv_linear_prologue": 0}, id_generic)
    _assert_within_bound(case, y1, "linear-pixel prologue")
    _assert_batchnorm_statistics(case, s1)
    assert _same_bits(y0, y1)
    f1 = _filled_slots(case, s1)
    assert bool(torch.isfinite(f1).all()) and _same_bits(f1, _filled_slots(case, s0))
    if id_lin & 1:                                             # several Cout chunks: the same tile on the 2-D grid (id bit 0 clear)
        y2, s2 = _conv(case, {"conv_xcd_pair": 0}, id_lin & ~1)
        assert _same_bits(y2, y1) and _same_bits(f1, _filled_slots(case, s2))


# ---------------------------------------------------------------------------------------------------------------------------
# VQ: tiles per wave T = 8, 4, 2, 1 against the chain oracle -- indices and the winning distance's bits
# ---------------------------------------------------------------------------------------------------------------------------
_VQ_REF = {}


def _vq_case(n, c, k, bf16=False):
    """(rows, codebook, oracle indices, oracle distances), computed once per shape"""
    from oracle import vq_chain
    key = (n, c, k, bf16)
    if key not in _VQ_REF:
        rows = synth.uniform(n * 7 + c, (n, c), -1.0, 1.0)
        if bf16:
            rows = rows.bfloat16().float()
        W = synth.uniform(k * 13 + c, (k, c), -1.0, 1.0)
        ref_i, ref_d = vq_chain.assign(rows.numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
        _VQ_REF[key] = (rows, W, ref_i, ref_d)
    return _VQ_REF[key]


def _vq_assign_and_compare(n, c, k, opts, want_t, bf16=False):
    from vq_seg_amd import _hip
    rows, W, ref_i, ref_d = _vq_case(n, c, k, bf16)
    rd = rows.to(dev())
    with _Options(opts):
        assert _hip.vq_tiles_per_wave(n, k) == want_t
        idx, dmin = _hip.vq_assign(rd.bfloat16() if bf16 else rd, W.to(dev()), want_dmin=True)
        torch.cuda.synchronize()
    idx, dmin = idx.cpu().numpy(), dmin.cpu().numpy()
    assert np.array_equal(idx, ref_i), f"T = {want_t}: {int((idx != ref_i).sum())} indices differ, first at row {int(np.argmax(idx != ref_i))}"
    assert np.array_equal(dmin.view(np.uint32), ref_d.view(np.uint32)), f"T = {want_t}: distance bits differ"
    return idx, dmin


def test_vq_every_tiles_per_wave_count_on_ragged_rows_and_codes():
    """N = 8100 (64 row groups, the last one 36 rows), C = 20 (off the 16-channel stage), K = 2040 (64 code tiles, the last one 24
    codes): the cap 8, 4, 2, 1 selects T = 8, 4, 2, 1; each equals the oracle in indices and distance bits, hence each other."""
    outs = [_vq_assign_and_compare(8100, 20, 2040, {"vq_max_tiles_per_wave": t}, t) for t in (8, 4, 2, 1)]
    for idx, dmin in outs[1:]:
        assert np.array_equal(idx, outs[0][0]) and np.array_equal(dmin.view(np.uint32), outs[0][1].view(np.uint32))


def test_vq_tile_count_that_eight_does_not_divide():
    """K = 1912: 60 code tiles, 60 % 8 != 0: T = 4 at default options"""
    _vq_assign_and_compare(8100, 20, 1912, {}, 4)


def test_vq_fine_split_and_the_earlier_rule_give_the_same_bits():
    """N = 32700 (256 row groups), C = 8, K = 2048: the fine split takes T = 4 (4096 workgroups), the earlier rule T = 8"""
    a = _vq_assign_and_compare(32700, 8, 2048, {"vq_fine_split": 1}, 4)
    b = _vq_assign_and_compare(32700, 8, 2048, {"vq_fine_split": 0}, 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_vq_every_tiles_per_wave_count_behind_the_bf16_filter():
    """bf16 rows at C = 32, K = 2048 (the candidate filter's shape conditions): the filter path launches (counter) and the exact
    re-score behind it runs at T = 8, 4, 2, 1 -- the same indices and distance bits as the oracle on the same bf16 values."""
    from vq_seg_amd import _hip
    for t in (8, 4, 2, 1):
        before = _hip.set_option("vq_filter_launches", 0)
        try:
            _vq_assign_and_compare(8100, 32, 2048, {"vq_max_tiles_per_wave": t}, t, bf16=True)
            took = _hip.set_option("vq_filter_launches", 0)
        finally:
            _hip.set_option("vq_filter_launches", before)
        assert took >= 1, "the bf16 rows did not take the candidate filter"
