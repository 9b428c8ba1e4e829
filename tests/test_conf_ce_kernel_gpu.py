"""The fused confidence-weighted CPS pass (vqseg_conf_ce_*; nnf.conf_ce / conf_ce_pair behind loss.conf_ce_loss) on the GPU, against the
float64 restatement of tests/conf_ce_cases.py on margin-clean inputs and against what the reference computed
(tests/golden/conf_ce_ref.npz).

Bars, those of tests/test_focal_gpu.py.  Forward: 2e-6 relative.  Gradients, with respect to the inputs and to the targets each: per
case the float32 torch-op form of the same loss (loss.conf_ce_loss on CPU tensors; for the golden cases the reference's own float32
gradient from the file) is measured against float64, and the kernel is allowed 4x that error plus one float32 ulp of the largest
gradient entry.  The clamp case is judged the same way; there the kernel, which never forms 1 - p by subtraction, is expected to be
the more accurate of the two.  Measured errors of both: profiles/conf_ce.md."""
import functools

import numpy as np
import pytest
import torch

from tests import conf_ce_cases as cc, golden_io

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PX_PER_BLOCK = 4096                                  # DICE_PX_PER_BLOCK (csrc/loss_kernels.h)
# (B, C, H, W): HW below a wave's 256-pixel stride; not a multiple of 256; one pixel over a block's span (two blocks and the fold)
SHAPES = [(3, 2, 9, 13), (3, 3, 17, 31), (3, 4, 17, 241), (3, 3, 17, 241)]
LAYOUTS = ["nchw", "channels_last"]
assert 17 * 241 == PX_PER_BLOCK + 1


def to_dev(v, layout):
    v = v.to(DEV)
    return v.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else v


def grads_of(fn, a, b, want_b=True):
    """-> value(s), gradients with respect to a and b of the sum of fn(a, b)'s outputs"""
    x = a.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    t = b.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = fn(x, t)
    total = y if torch.is_tensor(y) else sum(y)
    g = torch.autograd.grad(total, (x, t) if want_b else (x,), allow_unused=True)
    return y, g[0], (g[1] if want_b else None)


def launches(monkeypatch):
    from vq_seg_amd import nnf
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    return names


@functools.lru_cache(maxsize=None)
def reference(name, shape):
    """float64 restatement and the float32 torch-op yardstick of a case, made once on the CPU: (loss, gx, gt) each"""
    from vq_seg_amd.loss import conf_ce_loss
    a, b, _ = cc.inputs(name, shape)
    par = cc.params(name)
    ref = cc.restate_grads(a, b, *par)
    y, gx, gt = grads_of(lambda x, t: conf_ce_loss(x, t, True, *par), a, b)
    return ref, (y.detach(), gx, gt)


def check_forward(got, ref, what):
    err, bar = abs(float(got) - float(ref)), 2e-6 * abs(float(ref))
    print(f"{what}: forward {float(got):.9g} restated {float(ref):.9g} err {err:.3e} bar {bar:.3e}")
    assert err <= bar, what


def check_grad(got, ref, yard, what):
    ref = ref.cpu().double()
    k_err = float((got.cpu().double() - ref).abs().max())
    y_err = float((yard.cpu().double() - ref).abs().max())
    bar = 4 * y_err + float(np.spacing(np.float32(ref.abs().max())))
    print(f"{what}: gradient err kernel {k_err:.3e}, torch-op form {y_err:.3e}, bar {bar:.3e}, largest entry {float(ref.abs().max()):.3e}")
    assert k_err <= bar, what
    return k_err, y_err


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(cc.CASES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_fp64_restatement(shape, name, layout, monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import conf_ce_loss
    a, b, _ = cc.inputs(name, shape)
    par = cc.params(name)
    (r_loss, r_gx, r_gt), (_y, y_gx, y_gt) = reference(name, shape)
    xa, xb = to_dev(a, layout), to_dev(b, layout)
    assert nnf.conf_ce_supported(xa, xb)
    names = launches(monkeypatch)
    got, gx, gt = grads_of(lambda x, t: conf_ce_loss(x, t, True, *par), xa, xb)
    assert names == ["vqseg_conf_ce_forward_f", "vqseg_conf_ce_backward_f"]
    assert got.dtype == torch.float32 and got.dim() == 0
    assert gx.stride() == xa.stride() and gt.stride() == xb.stride()
    what = f"{name} {'x'.join(map(str, shape))} {layout}"
    check_forward(got, r_loss, what)
    kx, yx = check_grad(gx, r_gx, y_gx, what + " d/dx")
    check_grad(gt, r_gt, y_gt, what + " d/dt")
    parts = {}
    cc.restate(a, b, *par, parts=parts)
    st = dict(zip(nnf.CONF_CE_STATS, nnf.conf_ce_stats(xa, xb, *par)[0].tolist()))
    assert (st["m"], st["mn"]) == (parts["m"], parts["mn"])            # integer counts: exact on margin-clean inputs
    for k in ("sum_pos", "sum_neg", "sum_p2"):
        assert abs(st[k] - parts[k]) <= 2e-6 * abs(parts[k]), (k, st[k], parts[k])
    if name == "m0":                                                   # M == 0: an attached 0 with exactly-zero gradients
        assert float(got) == 0.0 and got.requires_grad and not bool(gx.any()) and not bool(gt.any())
    if name == "mn0":                                                  # Mn == 0: the negative term is exactly absent
        assert st["mn"] == 0 and st["sum_neg"] == 0.0 and st["inv_mn"] == 0.0 and bool(torch.isfinite(gx).all())
    if name == "clamp":                                                # clamped elements carry no negative-term gradient: covered by the bar;
        print(f"{what}: kernel / torch-op gradient error {kx / yx if yx else float('nan'):.3g}")     # the ratio goes to the profile


@functools.lru_cache(maxsize=None)
def golden():
    return golden_io.load("conf_ce_ref")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", cc.GOLDEN_CASES)
def test_against_the_reference_golden(name, layout):
    from vq_seg_amd.loss import conf_ce_loss
    fx = golden()
    a, b, _ = cc.golden_inputs(name)
    par = cc.params(name)
    got, gx, gt = grads_of(lambda x, t: conf_ce_loss(x, t, True, *par), to_dev(a, layout), to_dev(b, layout))
    what = f"golden {name} {layout}"
    if f"{name}_f64" in fx.meta["nan"]:                                # the reference is NaN (Mn == 0): the restatement stands in
        r_loss, r_gx, r_gt = cc.restate_grads(a, b, *par)
        _y, y_gx, y_gt = grads_of(lambda x, t: conf_ce_loss(x, t, True, *par), a, b)
        assert bool(torch.isfinite(got))
    elif f"{name}_f64" in fx.meta["no_graph"]:                         # the reference: a constant 0 (M == 0)
        assert float(fx[f"{name}_f64_loss"]) == 0.0 and float(got) == 0.0 and not bool(gx.any()) and not bool(gt.any())
        return
    else:
        r_loss, r_gx, r_gt = fx[f"{name}_f64_loss"], fx[f"{name}_f64_gx"], fx[f"{name}_f64_gt"]
        y_gx, y_gt = fx[f"{name}_f32_gx"], fx[f"{name}_f32_gt"]        # the yardstick: the reference's own float32 gradients
    check_forward(got, r_loss, what)
    check_grad(gx, r_gx, y_gx, what + " d/dx")
    check_grad(gt, r_gt, y_gt, what + " d/dt")


@pytest.mark.parametrize("layouts", [("nchw", "nchw"), ("channels_last", "channels_last"), ("nchw", "channels_last")], ids="-".join)
@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_pair_equals_two_single_calls_bit_for_bit(name, layouts, monkeypatch):
    from vq_seg_amd import nnf
    shape = (3, 3, 17, 241)
    a, b, _ = cc.inputs(name, shape)
    par = cc.params(name)
    xa, xb = to_dev(a, layouts[0]), to_dev(b, layouts[1])
    names = launches(monkeypatch)
    (l_ab, l_ba), ga, gb = grads_of(lambda x, t: nnf.conf_ce_pair(x, t, *par), xa, xb)
    assert names == ["vqseg_conf_ce_forward_f", "vqseg_conf_ce_backward_f"]             # one launch each way for both directions
    (s_ab, s_ba), sa, sb = grads_of(lambda x, t: (nnf.conf_ce(x, t, *par), nnf.conf_ce(t, x, *par)), xa, xb)
    assert torch.equal(l_ab, s_ab) and torch.equal(l_ba, s_ba)
    assert torch.equal(ga, sa) and torch.equal(gb, sb)
    assert ga.stride() == xa.stride() and gb.stride() == xb.stride()
    pst, sst = nnf.conf_ce_stats(xa, xb, *par, pair=True), torch.cat([nnf.conf_ce_stats(xa, xb, *par), nnf.conf_ce_stats(xb, xa, *par)])
    assert torch.equal(pst, sst)


@pytest.mark.parametrize("name", ["neg_t2", "clamp", "ref"])
def test_pair_with_upstream_scalars_is_the_restated_weighted_sum(name):
    """each direction scaled by its own upstream scalar, read on the device: where the unreliable weights enter"""
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import conf_ce_loss
    shape, (uw_a, uw_b) = (3, 3, 17, 241), (1.25, 1.0625)
    a, b, _ = cc.inputs(name, shape)
    par = cc.params(name)

    def weighted(one):
        return lambda x, t: uw_a * one(x, t) + uw_b * one(t, x)

    r_loss, r_ga, r_gb = grads_of(weighted(lambda x, t: cc.restate(x, t, *par)), a.double(), b.double())
    _y, y_ga, y_gb = grads_of(weighted(lambda x, t: conf_ce_loss(x, t, True, *par)), a, b)
    wa, wb = torch.tensor(uw_a, device=DEV), torch.tensor(uw_b, device=DEV)            # device scalars, as the trainer's are

    def pair(x, t):
        l_ab, l_ba = nnf.conf_ce_pair(x, t, *par)
        return wa * l_ab + wb * l_ba

    got, ga, gb = grads_of(pair, to_dev(a, "nchw"), to_dev(b, "channels_last"))
    check_forward(got, r_loss, f"weighted pair {name}")
    check_grad(ga, r_ga, y_ga, f"weighted pair {name} d/da")
    check_grad(gb, r_gb, y_gb, f"weighted pair {name} d/db")


@pytest.mark.parametrize("pair", [False, True], ids=["single", "pair"])
def test_detached_targets(pair):
    from vq_seg_amd import nnf
    a, b, _ = cc.inputs("neg", (3, 3, 17, 31))
    par = cc.params("neg")
    xa, xb = to_dev(a, "nchw"), to_dev(b, "channels_last")
    if not pair:
        y, gx, gt = grads_of(lambda x, t: nnf.conf_ce(x, t, *par, detach_targets=True), xa, xb)
        y2, gx2, gt2 = grads_of(lambda x, t: nnf.conf_ce(x, t, *par), xa, xb)
        assert gt is None and gt2 is not None and bool(gt2.any())      # not produced / the path through the weight
        assert torch.equal(y, y2) and torch.equal(gx, gx2)
    else:                                                              # each tensor keeps only its input-side gradient
        (l1, l2), ga, gb = grads_of(lambda x, t: nnf.conf_ce_pair(x, t, *par, detach_targets=True), xa, xb)
        _, sa, _n = grads_of(lambda x, t: nnf.conf_ce(x, t, *par, detach_targets=True), xa, xb)
        _, sb, _n = grads_of(lambda x, t: nnf.conf_ce(x, t, *par, detach_targets=True), xb, xa)
        assert torch.equal(ga, sa) and torch.equal(gb, sb)


def test_two_runs_give_the_same_bits():
    from vq_seg_amd import nnf
    a, b, _ = cc.inputs("neg_t2", (3, 4, 17, 241))
    par = cc.params("neg_t2")
    xa, xb = to_dev(a, "nchw"), to_dev(b, "nchw")
    for fn in (lambda x, t: nnf.conf_ce(x, t, *par), lambda x, t: nnf.conf_ce_pair(x, t, *par)):
        y1, g1, h1 = grads_of(fn, xa, xb)
        y2, g2, h2 = grads_of(fn, xa, xb)
        assert all(torch.equal(u, v) for u, v in zip(y1 if isinstance(y1, tuple) else (y1,), y2 if isinstance(y2, tuple) else (y2,)))
        assert torch.equal(g1, g2) and torch.equal(h1, h2)


def test_what_the_pass_does_not_take_stays_on_torch_ops(monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import conf_ce_loss
    a, b, _ = cc.inputs("neg", (3, 3, 17, 31))
    par = cc.params("neg")
    xa, xb = a.to(DEV), b.to(DEV)
    assert nnf.conf_ce_supported(xa, xb) and not nnf.conf_ce_supported(xa.double(), xb.double()) and not nnf.conf_ce_supported(xa, xb[:, :2])
    assert not nnf.conf_ce_supported(a, b) and not nnf.conf_ce_supported(xa, b)
    x5 = torch.cat([xa, xa[:, :2]], dim=1)
    assert not nnf.conf_ce_supported(x5, x5)
    names = launches(monkeypatch)
    got = conf_ce_loss(xa.double(), xb.double(), True, *par)           # float64 on the device: torch ops
    assert not names and got.dtype == torch.float64
    check_forward(got, cc.restate(a, b, *par), "float64 logits on the device (torch ops)")
    row = xa[:, :, :1, :].clone().requires_grad_(True)                 # overlapping memory (a broadcast row): copied, not written through
    y = nnf.conf_ce(row.expand(-1, -1, 17, -1), xb, *par)
    (g_row,) = torch.autograd.grad(y, row)
    y_ref, g_ref, _g = grads_of(lambda x, t: nnf.conf_ce(x, t, *par), row.detach().expand(-1, -1, 17, -1).contiguous(), xb)
    assert torch.equal(y.detach(), y_ref.detach()) and torch.allclose(g_row, g_ref.sum(dim=2, keepdim=True), rtol=1e-5, atol=1e-9)
