"""The three feature-perturbation entry points on the GPU (include/vqseg.h: vqseg_channel_keep_f, vqseg_channel_dropout_cat_f,
vqseg_channel_dropout_fold_f) against the torch restatement of their definition, bit for bit:

    draw      the torch-op Philox (nnf.channel_keep on the CPU: integer ops, tests/test_feature_perturb_cpu.py pins its known answers)
    forward   torch.cat((x, torch.where(scale == 0, 0, (x.float() * scale).to(dtype))))
    backward  torch.where(scale == 0, g[:B], (g[:B].float() + g[B:].float() * scale).to(dtype))     product, then sum, in float32

Shapes (B, C, H, W), each in float32 and bfloat16, NCHW-contiguous and channels_last:
    (1, 1, 1, 1)     the smallest case
    (2, 3, 5, 7)     a 16-byte unit spans pixels; the odd sample size (105 elements) puts the second sample and the second half off
                     16-byte alignment
    (3, 8, 4, 4)     exactly one bf16 unit per channels_last pixel
    (2, 20, 3, 3)    C no multiple of the unit
    (2, 64, 9, 3)    whole 1 KiB tiles and a partial last one
    (1, 264, 2, 2)   C above the 256 units of one workgroup iteration
NaN, +-Inf and -0.0 are planted in kept and in dropped channels of x and of g.  The guard-band cases run each entry point through
tests/extent.run_case (plain / 0xff / 0x00 surroundings) at a ragged, a smallest and a vector-path case."""
import pytest
import torch

from tests import extent as E
from vq_seg_amd import _hip, nnf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 1, 1), (2, 3, 5, 7), (3, 8, 4, 4), (2, 20, 3, 3), (2, 64, 9, 3), (1, 264, 2, 2)]
DTYPES = [torch.float32, torch.bfloat16]
FORMATS = [torch.contiguous_format, torch.channels_last]
SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0)
IDS = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", ""))


@pytest.mark.parametrize("sizes", [[(1, 1)], [(1, 7)], [(3, 64), (3, 257)], [(1, 4097)]], ids=["1", "7", "3x64+3x257", "4097"])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.9])
def test_the_draw_is_the_torch_op_philox(sizes, p, monkeypatch):
    key = dict(seed=(3 << 32) | 42, stream=5, step=(1 << 32) | 17)
    want, _ = nnf.channel_keep(sizes, p, device="cpu", **key)
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    flat, views = nnf.channel_keep(sizes, p, device=DEV, **key)
    torch.cuda.synchronize()
    assert names == ["vqseg_channel_keep_f"] and flat.is_cuda and [tuple(v.shape) for v in views] == sizes
    assert E.same_bits(flat, want), E.first_difference(flat, want)
    monkeypatch.setitem(_hip.PY_OPTS, "py_feature_perturb", 0)                       # the torch-op form on the device: the same table
    again, _ = nnf.channel_keep(sizes, p, device=DEV, **key)
    assert names == ["vqseg_channel_keep_f"] and again.is_cuda and E.same_bits(again, want)


def _scales(b, c):
    """scale tables of a case: draws at p = 0.5 (scale 2: exact) and p = 0.25 (scale 4/3: every product rounds) with a dropped
    first and a kept last entry; a single entry both ways"""
    if b * c == 1:
        return [torch.zeros(1, 1, device=DEV), torch.full((1, 1), 2.0, device=DEV), torch.full((1, 1), float(nnf.channel_keep_params(0.25)[1]), device=DEV)]
    out = []
    for p in (0.5, 0.25):
        flat, (view,) = nnf.channel_keep([(b, c)], p, 7, 1, b * c, DEV)
        flat[0], flat[-1] = 0.0, nnf.channel_keep_params(p)[1]
        out.append(view)
    return out


def _values(shape, dtype, fmt, scale, seed):
    """normal values with the specials planted in kept and in dropped channels (where the table has both)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    n, c, h, w = (shape[0] // scale.shape[0]) * scale.shape[0], shape[1], shape[2], shape[3]
    s = scale.cpu().repeat(shape[0] // scale.shape[0], 1)
    for want_kept in (True, False):
        where = [(i, k) for i in range(n) for k in range(c) if bool(s[i, k] != 0) == want_kept]
        for j, v in enumerate(SPECIALS if where else ()):
            i, k = where[(3 * j) % len(where)]
            x[i, k, j % h, (j // h) % w] = v
    return x.to(dtype).to(DEV).contiguous(memory_format=fmt)


def _forward(x, scale):
    s = scale[:, :, None, None]
    return torch.cat((x, torch.where(s == 0, torch.zeros((), dtype=x.dtype, device=x.device), (x.float() * s).to(x.dtype))))


def _backward(g, scale):
    n = g.shape[0] // 2
    s = scale[:, :, None, None]
    return torch.where(s == 0, g[:n], (g[:n].float() + g[n:].float() * s).to(g.dtype))


@pytest.mark.parametrize("fmt", FORMATS, **IDS)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("shape", SHAPES, **IDS)
def test_forward_and_backward_are_the_restatement_bit_for_bit(shape, dtype, fmt, monkeypatch):
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    b, c, h, w = shape
    for t, scale in enumerate(_scales(b, c)):
        x = _values(shape, dtype, fmt, scale, 100 + t).requires_grad_(True)
        assert nnf.channel_dropout_supported(x)
        out = nnf.channel_dropout_cat(x, scale)
        want = _forward(x.detach(), scale)
        assert out.shape == (2 * b, c, h, w) and out.dtype == dtype and out.is_contiguous(memory_format=fmt)
        assert E.same_bits(out.detach(), want), f"forward, table {t}: " + E.first_difference(out.detach(), want)
        assert E.same_bits(out.detach()[:b], x.detach())                                # the clean half: x by bits
        g = _values((2 * b, c, h, w), dtype, fmt, scale, 200 + t)
        (gx,) = torch.autograd.grad(out, x, g)
        want = _backward(g, scale)
        assert gx.shape == x.shape and gx.dtype == dtype
        assert E.same_bits(gx, want), f"backward, table {t}: " + E.first_difference(gx, want)
        dropped = (scale == 0)[:, :, None, None].expand(shape)
        if bool(dropped.any()):                                                        # selection: +0.0 forward, g[:B] alone backward
            assert int(E.as_ints(out.detach()[b:])[dropped].abs().sum()) == 0
            assert torch.equal(E.as_ints(gx)[dropped], E.as_ints(g[:b])[dropped])
        torch.cuda.synchronize()
    assert names.count("vqseg_channel_dropout_cat_f") == names.count("vqseg_channel_dropout_fold_f") == len(_scales(b, c))


@pytest.mark.parametrize("fmt", FORMATS, **IDS)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
@pytest.mark.parametrize("shape", [(2, 20, 3, 3), (2, 64, 9, 3)], **IDS)
def test_autograd_through_the_op_is_torchs_autograd_of_the_restatement(shape, dtype, fmt):
    """p = 0.5 (scale 2: the product is exact in either type) and finite gradients without a negative zero: there torch's own backward
    of the restated forward -- a multiply and an add as separate operators, each rounded to the tensor's type -- is the definition's"""
    b, c = shape[:2]
    _flat, (scale,) = nnf.channel_keep([(b, c)], 0.5, 11, 0, 3, DEV)
    assert 0 < int((scale == 0).sum()) < scale.numel()
    g0 = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=g0).to(dtype).to(DEV).contiguous(memory_format=fmt)
    g = torch.randn((2 * b,) + shape[1:], generator=g0).to(dtype).to(DEV).contiguous(memory_format=fmt)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out, ref = nnf.channel_dropout_cat(xa, scale), _forward(xb, scale)
    assert E.same_bits(out.detach(), ref.detach())
    (ga,), (gb,) = torch.autograd.grad(out, xa, g), torch.autograd.grad(ref, xb, g)
    assert E.same_bits(ga, gb), E.first_difference(ga, gb)
    # ... and under the A/B switch the torch-op form of the op gives the same bits both ways
    _hip.PY_OPTS["py_feature_perturb"] = 0
    try:
        xc = x.clone().requires_grad_(True)
        alt = nnf.channel_dropout_cat(xc, scale)
        (gc,) = torch.autograd.grad(alt, xc, g)
    finally:
        del _hip.PY_OPTS["py_feature_perturb"]
    assert E.same_bits(alt.detach(), out.detach()) and E.same_bits(gc, ga)


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


KEEP_CASES = [("ragged", 64 * 3 + 257 * 3), ("smallest", 1), ("two-blocks", 4097)]


@pytest.mark.parametrize("name,total", KEEP_CASES, ids=[c[0] for c in KEEP_CASES])
def test_extent_of_the_draw(name, total):
    L = _hip.lib()
    spec = dict(scale=E.Out(total, torch.float32, align=4))
    call = lambda t: L.vqseg_channel_keep_f(t["scale"].data_ptr(), total, 42, 1, 7, 1 << 31, 2.0, _stream())
    runs = E.run_case(spec, call, DEV, torch.cuda.synchronize, f"vqseg_channel_keep_f {name}")
    want, _ = nnf.channel_keep([(1, total)], 0.5, 42, 1, 7, "cpu")
    assert E.same_bits(runs[1]["scale"], want)


# (name, shape, dtype, channels_last, alignment of every pointer)
DROPOUT_CASES = [
    ("ragged-f32-nchw", (2, 3, 5, 7), torch.float32, 0, 4),
    ("ragged-bf16-cl", (2, 20, 3, 3), torch.bfloat16, 1, 2),
    ("smallest-f32", (1, 1, 1, 1), torch.float32, 1, 4),
    ("smallest-bf16", (1, 1, 1, 1), torch.bfloat16, 0, 2),
    ("vector-bf16-cl", (2, 64, 9, 3), torch.bfloat16, 1, 16),
    ("vector-f32-nchw", (2, 64, 9, 3), torch.float32, 0, 16),
]


def _storage(shape, dtype, cl, seed):
    """the tensor's elements in storage order, flat, and its logical (B, C, H, W) view"""
    b, c, h, w = shape
    flat = torch.randn(b * c * h * w, generator=torch.Generator().manual_seed(seed)).to(dtype)
    return flat


def _logical(flat, shape, cl):
    b, c, h, w = shape
    return flat.view(b, h, w, c).permute(0, 3, 1, 2) if cl else flat.view(b, c, h, w)


@pytest.mark.parametrize("name,shape,dtype,cl,align", DROPOUT_CASES, ids=[c[0] for c in DROPOUT_CASES])
def test_extent_of_forward_and_backward(name, shape, dtype, cl, align):
    L = _hip.lib()
    b, c, h, w = shape
    bf = int(dtype == torch.bfloat16)
    scale = _scales(b, c)[-1].cpu().contiguous()
    x = _storage(shape, dtype, cl, 1)
    spec = dict(x=E.In(x, align=align), scale=E.In(scale.reshape(-1), align=4), out=E.Out(2 * x.numel(), dtype, align=align))
    call = lambda t: L.vqseg_channel_dropout_cat_f(bf, t["x"].data_ptr(), t["scale"].data_ptr(), t["out"].data_ptr(), b, c, h, w, cl, _stream())
    runs = E.run_case(spec, call, DEV, torch.cuda.synchronize, f"vqseg_channel_dropout_cat_f {name}")
    want = _forward(_logical(x, shape, cl).to(DEV), scale.to(DEV))
    assert E.same_bits(_logical(runs[1]["out"], (2 * b, c, h, w), cl), want)
    g = _storage((2 * b, c, h, w), dtype, cl, 2)
    spec = dict(g=E.In(g, align=align), scale=E.In(scale.reshape(-1), align=4), gx=E.Out(x.numel(), dtype, align=align))
    call = lambda t: L.vqseg_channel_dropout_fold_f(bf, t["g"].data_ptr(), t["scale"].data_ptr(), t["gx"].data_ptr(), b, c, h, w, cl, _stream())
    runs = E.run_case(spec, call, DEV, torch.cuda.synchronize, f"vqseg_channel_dropout_fold_f {name}")
    want = _backward(_logical(g, (2 * b, c, h, w), cl).to(DEV), scale.to(DEV))
    assert E.same_bits(_logical(runs[1]["gx"], shape, cl), want)


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    L = _hip.lib()
    x, s, o = torch.zeros(8, device=DEV), torch.ones(2, device=DEV), torch.full((16,), 7.0, device=DEV)
    for args in ((2, x.data_ptr(), s.data_ptr(), o.data_ptr(), 1, 2, 2, 2, 0), (0, x.data_ptr(), s.data_ptr(), o.data_ptr(), 1, 2, 2, 2, 2),
                 (0, x.data_ptr(), s.data_ptr(), o.data_ptr(), 0, 2, 2, 2, 0), (0, x.data_ptr(), None, o.data_ptr(), 1, 2, 2, 2, 0),
                 (0, x.data_ptr(), s.data_ptr(), x.data_ptr(), 1, 2, 2, 2, 0)):
        assert L.vqseg_channel_dropout_cat_f(*args, _stream()) == -1
        assert L.vqseg_channel_dropout_fold_f(*args, _stream()) == -1
    for args in ((o.data_ptr(), 0, 0, 0, 0, 0, 1.0), (o.data_ptr(), 4, 0, 1 << 32, 0, 0, 1.0), (o.data_ptr(), 4, 0, 0, 0, 1 << 32, 1.0),
                 (o.data_ptr(), 4, 0, 0, 0, 0, 0.5), (o.data_ptr(), 4, 0, 0, 0, 0, float("inf")), (None, 4, 0, 0, 0, 0, 1.0)):
        assert L.vqseg_channel_keep_f(*args, _stream()) == -1
    torch.cuda.synchronize()
    assert torch.equal(o, torch.full((16,), 7.0, device=DEV))
    with pytest.raises(_hip.HipLibraryError, match="scale must be a float32"):
        nnf.channel_dropout_cat(torch.zeros(1, 2, 2, 2, device=DEV), torch.ones(1, 3, device=DEV))
    y = nnf.channel_dropout_cat(torch.ones(1, 2, 2, 4, device=DEV)[:, :, :, ::2], torch.ones(1, 2, device=DEV))     # not dense: the torch-op form
    assert y.shape == (2, 2, 2, 2) and bool((y == 1).all())
