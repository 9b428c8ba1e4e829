"""fp64 parity of every convolution geometry the benchmark's model runs (tests/layer_cases.py's census), through the C ABI, at the
smallest sizes that read back the benchmark-size instantiation:
  * forward, bf16: raw output within dispatch_cases.bound on every element, BatchNorm partials at _patch_case's bars;
  * data gradient, bf16, in the form nnf._dgrad picks for the layer (ring, shortcut, folded, classes, generic per concat source);
  * weight gradient, bf16, at the one-block size and, where the plan reaches 8 slabs of several tiles, at the eight-slab size (the
    XCD-aware 1-D grid, id bit 0): vqseg_conv2d_wgrad_f, then vqseg_conv2d_wgrad2_f with accumulate = 1 onto that result, at
    test_wgrad3x3_fused_taps' bar, max |gw - ref| < 2e-5 max |ref|;
  * fp32 forward, data and weight gradient of a 3x3 at 512 channels and a wide concat row at precise_cases.bound -- the per-tap weight
    gradient is the one whose slab sum goes through launch_wgrad_reduce and its 8192-workgroup cap (the LDS-DMA plans sum their slabs
    with reduce_partials_kernel, whose grid is not capped);
  * the same launches at the benchmark's own sizes over zero-filled buffers: the id read back equals the test size's, bit 0 aside.
Outputs are pre-filled with NaN and followed by guard rows, workspaces by 0xA5 guard bytes; `conv_last_variant` is zeroed before and
asserted after every launch.  Each check prints its worst error over its bound (pytest -s); profiles/layer_census.md records them."""
import pytest
import torch

from tests import fast_cases as fc
from tests import layer_cases as lc
from tests import precise_cases as pc
from tests import stem_cases
from tests import synth
from tests import test_dispatch_variants_gpu as tdv
from tests import test_precise_conv_gpu as tpc
from tests.test_nn_gpu import _wgrad_ref_by_taps, _wgrad_workspace, _wgrad_workspace_intact, rel

pytestmark = pytest.mark.gpu

GUARD = tpc.GUARD
GW_GUARD = 64                                               # elements behind gw
BAR = 2e-5
U = fc.U

dev, _lib, _nan_fill, _report, _st, _ptr = tdv.dev, tdv._lib, tdv._nan_like_fill, tpc._report, tpc._st, tpc._ptr

NAMES = [r.name for r in lc.ROWS]
WGRAD_NAMES = NAMES + [r.name for r in lc.EXTRA_WGRAD_ROWS]


def _options(name):
    return tdv._Options(lc.OPTIONS.get(name, {}))


def _nan_rows(rows, c, dtype=torch.bfloat16):
    return torch.full((rows, c), float("nan"), dtype=dtype, device=dev())


def _read_id(want, what):
    got = _lib().vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert got == want, f"{what}: dispatched {got:#x}, the census names {want:#x}"


# ---------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_forward_raw_output_and_batchnorm_partials(name):
    """vqseg_conv2d_f with the BatchNorm partials, as the training forward launches it"""
    row, size = lc.BY_NAME[name], lc.SIZES[name].fwd
    case = lc.fast_case(row, "fwd", size)
    x, wt = fc.operands(case)
    hi, _lo = tpc._pack(wt, 0, False)
    ho, wo = fc.out_size(case)
    with _options(name):
        y, stat = tpc._conv(x, row.c1, hi, None, (row.cout, row.k, row.stride, row.pad, row.reflect, 1, ho, wo), False, lc.IDS[name].fwd, stat=True)
    ref, _S = fc.reference(case)
    _report(f"{name} {size} {lc.IDS[name].fwd:#x} forward", y, ref, fc.limit(case))
    m, cout = ref.shape
    rps = 64 if cout >= 64 else 32
    assert bool(torch.isfinite(stat[:(m + rps - 1) // rps]).all())
    tdv._assert_batchnorm_statistics_of(ref, stat)


# ---------------------------------------------------------------------------------------------------------------------------
# data gradient
# ---------------------------------------------------------------------------------------------------------------------------
def _sources(row):
    return [(0, row.c1), (row.c1, row.c2)] if row.c2 else [(0, row.c1)]


def _dgrad_generic(name, row, size, extra=False):
    """one vqseg_conv2d_f launch per concat source over gy with that source's transposed, tap-flipped image (nnf._dgrad_generic);
    extra: vqseg_conv2d_affine_f with unit scale, zero shift and a bf16 addend instead (nnf._dgrad_shortcut)"""
    n, h, w = size
    case = lc.fast_case(row, "dgrad", size)
    gy, wt = fc.operands(case)
    ref, S = fc.reference(case)
    limit, K = fc.limit(case), fc.contraction(case)
    assert fc.grad_grid(case) == (h, w, row.k - 1 - row.pad)
    for (c_lo, c_cnt), want_id in zip(_sources(row), lc.IDS[name].dgrad):
        thi, _lo = tpc._pack(wt[:, c_lo:c_lo + c_cnt].contiguous(), 1, False)
        geom = (c_cnt, row.k, 1, row.k - 1 - row.pad, False, 1, h, w)
        cols = slice(c_lo, c_lo + c_cnt)
        if not extra:
            with _options(name):
                gx, _ = tpc._conv(gy, row.cout, thi, None, geom, False, want_id)
            _report(f"{name} {size} {want_id:#x} data gradient, channels {c_lo} .. {c_lo + c_cnt}", gx, ref[:, cols], limit[:, cols])
            continue
        # the kernel rounds t = acc * 1 + 0 to bf16, adds the bf16 addend in fp32 and rounds again: fast_cases.epilogue_reference's
        # bound at unit scale, 2^-8 |y_ref| + 2^-8 |t_ref| + K 2^-23 S
        other = synth.uniform(777 + c_cnt, (n * h * w, c_cnt), -1, 1).bfloat16()
        res = torch.cat([other, torch.zeros(GUARD, c_cnt, dtype=torch.bfloat16)]).to(dev())
        one, zero = torch.ones(c_cnt, device=dev()), torch.zeros(c_cnt, device=dev())
        with _options(name):
            gx, _ = tpc._conv(gy, row.cout, thi, None, geom, False, want_id, affine=(one, zero, res, False))
        total = ref[:, cols] + other.double()
        _report(f"{name} {size} {want_id:#x} data gradient + shortcut gradient", gx, total, 2.0 ** -8 * total.abs() + 2.0 ** -8 * ref[:, cols].abs() + K * U * S[:, cols])


def _dgrad_ring(name, row, size):
    """nnf._dgrad_ring: the zero-padded gradient on the input grid (vqseg_conv2d_f), then vqseg_reflect_ring_f folds the border ring
    of the padded grid's gradient onto rows 1 / h - 2 and columns 1 / w - 2 in place.

    Reference: the fp64 gradient on the PADDED grid (fast_cases.reference of the reflect case), whose interior is the zero-padded
    gradient and whose reflect fold (stem_cases.reflect_fold: autograd of F.pad) is the gradient of the input.  Bounds: every padded
    position p within b_p = dispatch_cases.bound (its accumulation and its rounding to bf16, in gx or in the ring buffer); a pixel that
    gathers t > 1 positions sums them in fp32 and rounds once -- fast_cases.fold_reference's  E + 2^-8 (|sum ref_p| + E),
    E = sum b_p + (t - 1) 2^-23 sum (|ref_p| + b_p)."""
    L = _lib()
    n, h, w = size
    cin = row.c1
    case = lc.fast_case(row, "dgrad", size)
    gy, wt = fc.operands(case)
    ref, _S = fc.reference(case)
    b = fc.limit(case)
    assert fc.grad_grid(case) == (h + 2, w + 2, 2)
    grid = lambda v: v.reshape(n, h + 2, w + 2, cin)
    thi, _lo = tpc._pack(wt, 1, False)
    id_conv, id_ring = lc.IDS[name].dgrad
    with _options(name):
        g0, _ = tpc._conv(gy, row.cout, thi, None, (cin, 3, 1, 1, False, 1, h, w), False, id_conv)
    inner = lambda v: grid(v)[:, 1:-1, 1:-1].reshape(-1, cin)
    _report(f"{name} {size} {id_conv:#x} zero-padded data gradient", g0, inner(ref), inner(b))
    rl = stem_cases.ring_len(h, w)
    ring = _nan_rows(n * rl + GUARD, cin)
    gx = _nan_rows(n * h * w + GUARD, cin)
    gx[:n * h * w] = g0
    gyd = gy.bfloat16().to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    with _options(name):
        rc = L.vqseg_reflect_ring_f(gyd.data_ptr(), thi.data_ptr(), ring.data_ptr(), gx.data_ptr(), n, h, w, row.cout, cin, _st())
    assert rc == 0, L.vqseg_last_error()
    _read_id(id_ring, f"{name} ring")
    assert _nan_fill(ring[n * rl:]) and _nan_fill(gx[n * h * w:]), "the ring launch wrote behind a buffer"
    fold = stem_cases.reflect_fold
    t = fold(torch.ones(n, h + 2, w + 2, cin, dtype=torch.float64))
    want, fb, fa = fold(grid(ref)), fold(grid(b.expand_as(ref))), fold(grid(ref.abs() + b))
    e = fb + (t - 1) * U * fa
    limit = torch.where(t > 1, e + 2.0 ** -8 * (want.abs() + e), fb)
    assert int(t.max()) == 4 and bool((t[:, 2:-2, 2:-2] == 1).all())
    _report(f"{name} {size} {id_ring:#x} gradient through the reflect padding", gx[:n * h * w].reshape(n, h, w, cin), want, limit)


def _dgrad_folded(name, row, size):
    """vqseg_conv2d_dgrad_s2_fold_f as test_fast_conv_gpu's merged-fold test runs it; reference and bound: fast_cases.fold_reference"""
    L = _lib()
    n, h, w = size
    case = lc.fast_case(row, "fold", size)
    gy, wt = fc.operands(case)
    hi, _lo = tpc._pack_s2(wt)
    want, limit = fc.fold_reference(case)
    rows = int(L.vqseg_conv2d_dgrad_s2_fold_rows(n, h, w, int(row.reflect)))
    buf = _nan_rows(rows + GUARD, row.c1)
    gyd = gy.bfloat16().to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_dgrad_s2_fold_f(gyd.data_ptr(), hi.data_ptr(), buf.data_ptr(), n, h // 2, w // 2, row.cout, row.c1, h, w, int(row.reflect), _st())
    assert rc == 0, L.vqseg_last_error()
    (want_id,) = lc.IDS[name].dgrad
    _read_id(want_id, f"{name} merged fold")
    assert _nan_fill(buf[rows:]), "the launch wrote behind the rows vqseg_conv2d_dgrad_s2_fold_rows asks for"
    gx = buf[:n * h * w]
    assert bool(torch.isfinite(gx).all())
    _report(f"{name} {size} {want_id:#x} one-launch stride-2 data gradient", gx, want, limit)


def _dgrad_classes(name, row, size):
    """vqseg_conv2d_dgrad_s2_f(k = 1, accumulate = 1) onto the other consumer's gradient (nnf._dgrad_s2_classes with a fan-in deposit):
    test_fast_conv_gpu's bound, 2^-8 |other + ref| + 2^-8 |ref| + K 2^-23 S; pixels no gradient reaches keep `other` bit for bit"""
    L = _lib()
    n, h, w = size
    case = lc.fast_case(row, "dgrad", size)
    gy, wt = fc.operands(case)
    ref, S = fc.reference(case)
    hi, _lo = tpc._pack_s2(wt)
    ho, wo = fc.out_size(case)
    m = n * h * w
    other = synth.uniform(4242 + row.c1, (m, row.c1), -1, 1).bfloat16()
    gx = _nan_rows(m + GUARD, row.c1)
    gx[:m] = other.to(dev())
    gyd = gy.bfloat16().to(dev())
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_dgrad_s2_f(gyd.data_ptr(), hi.data_ptr(), None, gx.data_ptr(), n, ho, wo, row.cout, row.c1, 1, h, w, 0, 1, _st())
    assert rc == 0, L.vqseg_last_error()
    (want_id,) = lc.IDS[name].dgrad
    _read_id(want_id, f"{name} parity class")
    assert _nan_fill(gx[m:]), "the launch wrote behind the last gradient row"
    total = other.double() + ref
    _report(f"{name} {size} {want_id:#x} 1x1 stride-2 data gradient, accumulating", gx[:m], total, 2.0 ** -8 * total.abs() + 2.0 ** -8 * ref.abs() + fc.contraction(case) * U * S)
    odd = ((torch.arange(h)[:, None] % 2 == 1) | (torch.arange(w)[None, :] % 2 == 1)).repeat(n, 1, 1).reshape(-1)
    assert bool((S[odd] == 0).all()) and tdv._same_bits(gx[:m].cpu()[odd], other[odd])


@pytest.mark.parametrize("name", NAMES)
def test_data_gradient_in_the_form_the_step_takes(name):
    row, size = lc.BY_NAME[name], lc.SIZES[name].dgrad
    assert len(lc.IDS[name].dgrad) == {"ring": 2, "generic": len(_sources(row))}.get(row.dgrad, 1)
    if row.dgrad == "ring":
        _dgrad_ring(name, row, size)
    elif row.dgrad == "folded":
        _dgrad_folded(name, row, size)
    elif row.dgrad == "classes":
        _dgrad_classes(name, row, size)
    else:
        _dgrad_generic(name, row, size, extra=row.dgrad == "shortcut")


# ---------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------------------------
def _wgrad_launch(row, size, x, gy, gw, ws, nbytes, two_uses, accumulate, precise, want_id, what):
    """vqseg_conv2d_wgrad_f over the batch, or vqseg_conv2d_wgrad2_f over its first image and the rest as two uses of the layer"""
    L = _lib()
    n, h, w = size
    cin = row.c1 + row.c2
    ho, wo = lc.out_size(row, size)
    src = []
    for lo, hi in ([(0, 1), (1, n)] if two_uses else [(0, n)]):
        xs = x[lo:hi]
        src.append((gy[lo:hi].contiguous(), xs[..., :row.c1].contiguous(), xs[..., row.c1:].contiguous() if row.c2 else None, hi - lo))
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    tail = (row.c1, h, w, cin, ho, wo, row.cout, row.k, row.k, row.stride, row.pad, int(row.reflect), int(precise), cin, 0, int(accumulate),
            ws.data_ptr(), nbytes, gw.data_ptr(), _st())
    if two_uses:
        (ga, xa, xa2, na), (gb, xb, xb2, nb) = src
        rc = L.vqseg_conv2d_wgrad2_f(ga.data_ptr(), xa.data_ptr(), _ptr(xa2), na, gb.data_ptr(), xb.data_ptr(), _ptr(xb2), nb, *tail)
    else:
        ((ga, xa, xa2, na),) = src
        rc = L.vqseg_conv2d_wgrad_f(ga.data_ptr(), xa.data_ptr(), _ptr(xa2), row.c1, n, *tail[1:])
    assert rc == 0, L.vqseg_last_error()
    _read_id(want_id, what)
    numel = row.cout * cin * row.k * row.k
    assert _wgrad_workspace_intact(ws, nbytes), f"{what}: the launch wrote behind its workspace"
    assert _nan_fill(gw[numel:]), f"{what}: the launch wrote behind the gradient"
    return gw[:numel].reshape(row.cout, cin, row.k, row.k)


def _wgrad_buffers(row, size):
    L = _lib()
    n, h, w = size
    cin = row.c1 + row.c2
    ho, wo = lc.out_size(row, size)
    nbytes = L.vqseg_conv2d_wgrad_workspace_bytes(n, h, w, cin, ho, wo, row.cout, row.k, row.k)
    gw = torch.full((row.cout * cin * row.k * row.k + GW_GUARD,), float("nan"), dtype=torch.float32, device=dev())
    return gw, _wgrad_workspace(nbytes), nbytes


WGRAD_PARAMS = [(name, which) for name in WGRAD_NAMES for which in ("wgrad", "wgrad8") if getattr(lc.SIZES[name], which) is not None]


@pytest.mark.parametrize("name,which", WGRAD_PARAMS, ids=[f"{n}-{'eight-slabs' if w == 'wgrad8' else 'one-block'}" for n, w in WGRAD_PARAMS])
def test_weight_gradient_then_two_uses_accumulating(name, which):
    """gw (NaN-filled) = the gradient, then gw += the same gradient over two uses: both at 2e-5 of scale against fp64 on the same bf16
    values.  The eight-slab size reads back the one-block id with bit 0 set: the XCD-aware 1-D grid, `q % t_all` over the row's tiles."""
    row, size = lc.BY_NAME[name], getattr(lc.SIZES[name], which)
    want_id = lc.IDS[name].wgrad | (which == "wgrad8")
    cot, cit, tiles = lc.wgrad_tiles(row)
    assert (want_id >> 16 & 15, want_id >> 12 & 15) == (cot, cit)
    if name in ("d1.1", "l4.conv2", "l4.0.conv2", "d2.0", "d1.0", "d0.0", "d0.1"):
        assert row.cout * 9 * (row.c1 + row.c2) > lc.REDUCE_CAP           # more slab elements than 8192 workgroups of 256 threads
    if which == "wgrad8":
        assert tiles > 1
    x, gy = lc.wgrad_operands(row, size)
    ref = _wgrad_ref_by_taps(x, gy, row.k, row.stride, row.reflect)
    xd, gyd = x.bfloat16().to(dev()), gy.bfloat16().to(dev())
    gw, ws, nbytes = _wgrad_buffers(row, size)
    what = f"{name} {size} {want_id:#x} weight gradient, {tiles} tile{'s' * (tiles > 1)}"
    first = rel(_wgrad_launch(row, size, xd, gyd, gw, ws, nbytes, False, 0, False, want_id, what), ref)
    print(f"{what}: error / bar {first / BAR:.3g}")
    assert first < BAR
    second = rel(_wgrad_launch(row, size, xd, gyd, gw, ws, nbytes, True, 1, False, want_id, what + ", two uses"), 2 * ref)
    print(f"{what}, two uses onto it: error / bar {second / BAR:.3g}")
    assert second < BAR


# ---------------------------------------------------------------------------------------------------------------------------
# fp32
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.PRECISE_ROWS)
def test_precise_forward_data_gradient_and_weight_gradient(name):
    """conv_igemm_kernel<128, true, 32> and conv_wgrad_kernel<4, 4, true> at the census' channel counts, full-mantissa operands, at
    precise_cases.bound.  The weight gradient's slab has more than 8192 * 256 elements: wgrad_reduce_kernel's threads take a second trip
    through their grid-stride loop.  Then the same gradient over two uses with accumulate = 1: twice the bound, plus 2^-23 |2 ref| for
    the fp32 add."""
    row, size = lc.BY_NAME[name], lc.PRECISE_SIZE
    n, h, w = size
    cin = row.c1 + row.c2
    ids = lc.PRECISE_IDS
    case = lc.precise_case(row, "fwd", size)
    x, wt = pc.operands(case)
    hi, lo = tpc._pack(wt, 0, True)
    y, stat = tpc._conv(x, row.c1, hi, lo, (row.cout, row.k, row.stride, row.pad, row.reflect, 1, h, w), True, ids.fwd, stat=True)
    ref, S = pc.reference(case)
    _report(f"{name} {size} fp32 forward", y, ref, pc.bound(ref, S, pc.contraction(case)))
    tdv._assert_batchnorm_statistics_of(ref, stat)

    case = lc.precise_case(row, "dgrad", size)
    gy, wt = pc.operands(case)
    ref, S = pc.reference(case)
    limit = pc.bound(ref, S, pc.contraction(case))
    assert pc.grad_grid(case) == (h, w, 1)
    for (c_lo, c_cnt), want_id in zip(_sources(row), ids.dgrad):
        thi, tlo = tpc._pack(wt[:, c_lo:c_lo + c_cnt].contiguous(), 1, True)
        gx, _ = tpc._conv(gy, row.cout, thi, tlo, (c_cnt, 3, 1, 1, False, 1, h, w), True, want_id)
        _report(f"{name} {size} fp32 data gradient, channels {c_lo} .. {c_lo + c_cnt}", gx, ref[:, c_lo:c_lo + c_cnt], limit[:, c_lo:c_lo + c_cnt])

    assert row.cout * 9 * cin > lc.REDUCE_CAP
    case = lc.precise_case(row, "wgrad", size)
    x, gy, _prev = pc.operands(case)
    ref, S = pc.reference(case)
    limit = pc.bound(ref, S, pc.contraction(case))
    gw, ws, nbytes = _wgrad_buffers(row, size)
    xd, gyd = x.to(dev()), gy.to(dev())
    got = _wgrad_launch(row, size, xd, gyd, gw, ws, nbytes, False, 0, True, ids.wgrad, f"{name} fp32 weight gradient")
    _report(f"{name} {size} fp32 weight gradient", pc.to_rows(case, got), ref, limit)
    got = _wgrad_launch(row, size, xd, gyd, gw, ws, nbytes, True, 1, True, ids.wgrad, f"{name} fp32 weight gradient, two uses")
    _report(f"{name} {size} fp32 weight gradient, two uses onto it", pc.to_rows(case, got), 2 * ref, 2 * limit + pc.U * (2 * ref).abs())


# ---------------------------------------------------------------------------------------------------------------------------
# the benchmark's own sizes
# ---------------------------------------------------------------------------------------------------------------------------
def _zeros(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype, device=dev())


def _bench_conv(n, h, w, c1, cin, cout, k, stride, pad, reflect, ho, wo, stat, res=False):
    """one vqseg_conv2d_f / vqseg_conv2d_affine_f launch over zero-filled buffers -> the id it read back"""
    L = _lib()
    x1 = _zeros(n * h * w, c1)
    x2 = _zeros(n * h * w, cin - c1) if c1 < cin else None
    hi = _zeros(L.vqseg_conv_packed_elems(cout, cin, k, k, 0), dtype=torch.int16)
    m = n * ho * wo
    y = _zeros(m, cout)
    st_t = _zeros(L.vqseg_conv_stat_slots(m, cout), 2, cout, dtype=torch.float32) if stat else None
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    if res:
        one, zero, r = torch.ones(cout, device=dev()), _zeros(cout, dtype=torch.float32), _zeros(m, cout)
        rc = L.vqseg_conv2d_affine_f(x1.data_ptr(), _ptr(x2), c1, hi.data_ptr(), None, one.data_ptr(), zero.data_ptr(), r.data_ptr(), 0, y.data_ptr(),
                                     n, h, w, cin, cout, k, k, stride, pad, int(reflect), ho, wo, 0, _st())
    else:
        rc = L.vqseg_conv2d_f(x1.data_ptr(), _ptr(x2), c1, hi.data_ptr(), None, y.data_ptr(), _ptr(st_t), n, h, w, cin, cout, k, k, stride, pad,
                              int(reflect), 1, ho, wo, 0, _st())
    assert rc == 0, L.vqseg_last_error()
    got = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    return got


def _bench_dgrad(row):
    L = _lib()
    n, h, w = row.bench
    ho, wo = lc.out_size(row, row.bench)
    cin = row.c1 + row.c2
    if row.dgrad in ("generic", "shortcut"):
        return tuple(_bench_conv(n, h, w, row.cout, row.cout, c_cnt, row.k, 1, row.k - 1 - row.pad, False, h, w, False, res=row.dgrad == "shortcut")
                     for _c_lo, c_cnt in _sources(row))
    gy = _zeros(n * ho * wo, row.cout)
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    if row.dgrad == "ring":
        first = _bench_conv(n, h, w, row.cout, row.cout, cin, 3, 1, 1, False, h, w, False)
        thi = _zeros(L.vqseg_conv_packed_elems(row.cout, cin, 3, 3, 1), dtype=torch.int16)
        ring, gx = _zeros(n * stem_cases.ring_len(h, w), cin), _zeros(n * h * w, cin)
        rc = L.vqseg_reflect_ring_f(gy.data_ptr(), thi.data_ptr(), ring.data_ptr(), gx.data_ptr(), n, h, w, row.cout, cin, _st())
    elif row.dgrad == "folded":
        first = None
        hi = _zeros(L.vqseg_conv_packed_s2_elems(row.cout, cin, 3), dtype=torch.int16)
        buf = _zeros(int(L.vqseg_conv2d_dgrad_s2_fold_rows(n, h, w, int(row.reflect))), cin)
        rc = L.vqseg_conv2d_dgrad_s2_fold_f(gy.data_ptr(), hi.data_ptr(), buf.data_ptr(), n, ho, wo, row.cout, cin, h, w, int(row.reflect), _st())
    else:
        first = None
        hi = _zeros(L.vqseg_conv_packed_s2_elems(row.cout, cin, 1), dtype=torch.int16)
        gx = _zeros(n * h * w, cin)
        rc = L.vqseg_conv2d_dgrad_s2_f(gy.data_ptr(), hi.data_ptr(), None, gx.data_ptr(), n, ho, wo, row.cout, cin, 1, h, w, 0, 1, _st())
    assert rc == 0, L.vqseg_last_error()
    got = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    return (got,) if first is None else (first, got)


@pytest.mark.parametrize("name", NAMES)
def test_the_benchmark_size_takes_the_instantiation_the_parity_tests_ran(name):
    """Default options, zero-filled buffers, no reference: the forward launch, the data-gradient launches and the weight gradient over
    two uses of the benchmark's batch read back the census' ids, bit 0 (the grid mapping) aside -- or the id layer_cases.EXCEPTIONS
    names.  A retuned dispatch fails here until the census follows it."""
    row = lc.BY_NAME[name]
    n, h, w = row.bench
    ho, wo = lc.out_size(row, row.bench)
    cin = row.c1 + row.c2
    ids = lc.IDS[name]
    got = {"fwd": _bench_conv(n, h, w, row.c1, cin, row.cout, row.k, row.stride, row.pad, row.reflect, ho, wo, True)}
    torch.cuda.empty_cache()
    got["dgrad"] = _bench_dgrad(row)
    torch.cuda.empty_cache()
    size = (2 * n, h, w)
    gw, ws, nbytes = _wgrad_buffers(row, size)
    gw.zero_()
    x, gy = _zeros(2 * n, h, w, cin), _zeros(2 * n, ho, wo, row.cout)
    xa, xb = x[:n, ..., :row.c1].contiguous(), x[n:, ..., :row.c1].contiguous()      # (kept alive until the launch has run)
    xa2, xb2 = (x[:n, ..., row.c1:].contiguous(), x[n:, ..., row.c1:].contiguous()) if row.c2 else (None, None)
    L = _lib()
    assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0
    rc = L.vqseg_conv2d_wgrad2_f(gy[:n].data_ptr(), xa.data_ptr(), _ptr(xa2), n, gy[n:].data_ptr(), xb.data_ptr(), _ptr(xb2), n,
                                 row.c1, h, w, cin, ho, wo, row.cout, row.k, row.k, row.stride, row.pad, int(row.reflect), 0, cin, 0, 1,
                                 ws.data_ptr(), nbytes, gw.data_ptr(), _st())
    assert rc == 0, L.vqseg_last_error()
    got["wgrad"] = L.vqseg_set_option(b"conv_last_variant", 0)
    torch.cuda.synchronize()
    assert _wgrad_workspace_intact(ws, nbytes)
    print(f"{name} at {row.bench}: forward {got['fwd']:#x}, data gradient {', '.join(f'{v:#x}' for v in got['dgrad'])}, weight gradient {got['wgrad']:#x}")
    exc = lc.EXCEPTIONS.get(name)
    if exc is not None and exc[0] == "fwd":
        assert got["fwd"] == exc[1], f"forward {got['fwd']:#x}"
    else:
        assert got["fwd"] & ~1 == ids.fwd & ~1, f"forward {got['fwd']:#x}, the census ran {ids.fwd:#x}"
    if exc is not None and exc[0] == "dgrad":
        assert got["dgrad"] == (exc[1],), [hex(v) for v in got["dgrad"]]
    else:
        assert tuple(v & ~1 for v in got["dgrad"]) == tuple(v & ~1 for v in ids.dgrad), [hex(v) for v in got["dgrad"]]
    assert got["wgrad"] & ~1 == ids.wgrad & ~1, f"weight gradient {got['wgrad']:#x}, the census ran {ids.wgrad:#x}"
    bit0 = lc.SIZES[name].wgrad8 is not None
    assert got["wgrad"] & 1 == int(bit0), "the benchmark's grid kind is not the one the census records for the row"
