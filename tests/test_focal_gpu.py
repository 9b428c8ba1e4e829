"""The fused focal pass (vqseg_focal_*; nnf.focal behind loss.focal_loss / loss.FocalLoss) on the GPU.

Against tests/golden/focal_ref.npz -- what the reference's loss package computed -- for every golden case in both layouts, and
against an fp64 restatement of the reference arithmetic (written below) at the shapes where the kernel can go wrong.

Bars.  Forward values: 2e-6 relative, the bar of the fused CE + Dice sums (losses_metrics.npz).  For the per-pixel map of
reduction 'none' the 2e-6 is relative to the map's largest entry: a pixel whose p_t rounds to 1 in float32 has a loss of the size
of one ulp of 1, which no float32 evaluation -- the reference's `1 - p` and `log p` least of all -- resolves relative to itself.
Gradients: no number fixed in advance.  Per case the float32 torch-op form of the same loss (for the golden cases: the reference's
own gradient from the file) is measured against the fp64 restatement, and the kernel is allowed 4x that error plus one float32 ulp
of the largest gradient entry: both sum in an order of their own.  Measured errors of both: profiles/focal_loss.md (the kernel: 1.1 x
the torch-op form's in the median, 3.2 x at most, 0.73 of the bar in the worst case)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import golden_io, loss_cases as lc, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PX_PER_BLOCK = 4096                                  # DICE_PX_PER_BLOCK (csrc/loss_kernels.h)
# (C, H, W): HW below 256; not a multiple of 256; one pixel over a block's span (two blocks and the fold)
SHAPES = [(2, 9, 13), (3, 17, 31), (4, 17, 241), (3, 17, 241)]
GAMMAS = [0, 1, 2, 3, 2.5]
B, IGNORE, ALPHA = 3, 255, 0.25
assert 17 * 241 == PX_PER_BLOCK + 1


def restate(logits, target, alpha, gamma, ignore, weight, pre_softmax):
    """loss/focal_loss.py:9-33 (and FocalLoss.forward:62-68 with `pre_softmax`) in float64 -> the (B, HW) map"""
    b, c = logits.shape[:2]
    x = logits.double().reshape(b, c, -1)
    t = target.reshape(b, -1)
    keep = t != ignore
    if pre_softmax:
        x = torch.softmax(x, dim=1)
    p = torch.softmax(x * keep[:, None], dim=1)
    onehot = F.one_hot(t * keep, c).permute(0, 2, 1).double()
    if weight is not None:
        onehot = onehot * weight.double()[None, :, None]
    return (alpha * (1 - p) ** gamma * -torch.log(p) * onehot).sum(dim=1)


def reduce_(m, reduction):
    return m if reduction == "none" else m.sum() if reduction == "sum" else m.mean()


def value_and_grad(fn, logits, cot):
    x = logits.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = fn(x)
    (g,) = torch.autograd.grad(y if y.dim() == 0 else (y * cot.to(y.device, y.dtype)).sum(), x)
    return y.detach(), g


def check(got, got_grad, ref, ref_grad, yard_grad, what, report=None):
    """forward 2e-6 relative (map: of its largest entry); gradient within 4x the yardstick's own error + one ulp"""
    ref, got = ref.cpu().double(), got.cpu().double()
    fwd_err = float((got - ref).abs().max())
    fwd_bar = 2e-6 * float(ref.abs().max())
    ref_grad = ref_grad.cpu().double()
    k_err = float((got_grad.cpu().double() - ref_grad).abs().max())
    y_err = float((yard_grad.cpu().double() - ref_grad).abs().max())
    bar = 4 * y_err + float(np.spacing(np.float32(ref_grad.abs().max())))
    print(f"{what}: forward err {fwd_err:.3e} (bar {fwd_bar:.3e}); gradient err kernel {k_err:.3e}, torch-op form {y_err:.3e}, bar {bar:.3e}")
    if report is not None:
        report.append((what, fwd_err, fwd_bar, k_err, y_err, bar))
    assert fwd_err <= fwd_bar, what
    assert k_err <= bar, what


@functools.lru_cache(maxsize=None)
def case_inputs(c, h, w):
    """image 0: ~20 % ignored pixels; image 1: every pixel ignored; image 2: none"""
    seed = 1000 * c + h + w
    logits = synth.uniform(seed, (B, c, h, w), -8.0, 8.0)
    target = synth.labels(seed + 1, (B, h, w), c)
    target[0][synth.uniform(seed + 2, (h, w)) < 0.2] = IGNORE
    target[1] = IGNORE
    cot = synth.uniform(seed + 3, (B, h * w), -1.0, 1.0)
    weight = synth.uniform(seed + 4, (c,), 0.3, 1.0)
    return logits, target, cot, weight


def launches(monkeypatch):
    from vq_seg_amd import nnf
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    return names


@pytest.mark.parametrize("pre_softmax", [False, True], ids=["function", "module"])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("c,h,w", SHAPES)
def test_against_the_fp64_restatement(c, h, w, gamma, pre_softmax, monkeypatch):
    from vq_seg_amd.loss import FocalLoss, focal_loss
    from vq_seg_amd.loss.focal_loss import _focal_torch
    logits, target, cot, weight = case_inputs(c, h, w)
    names = launches(monkeypatch)
    for weighted in (False, True):
        wt = weight if weighted else None
        # the weighted arm in channels_last, with the weights already on the device; the other in NCHW
        x_dev = logits.to(DEV).contiguous(memory_format=torch.channels_last) if weighted else logits.to(DEV)
        w_dev = wt.to(DEV) if weighted else None
        for reduction in ("sum", "mean", "none"):
            if pre_softmax:
                fn = FocalLoss(c, ALPHA, gamma, IGNORE, reduction, w_dev)
                hip = lambda x: fn(x, target.to(DEV))                                                # noqa: E731
                yard = lambda x: _focal_torch(torch.softmax(x, 1), target, ALPHA, gamma, c, IGNORE, reduction, wt)      # noqa: E731
            else:
                hip = lambda x: focal_loss(x, target.to(DEV), ALPHA, gamma, c, IGNORE, reduction, w_dev)     # noqa: E731
                yard = lambda x: _focal_torch(x, target, ALPHA, gamma, c, IGNORE, reduction, wt)     # noqa: E731
            ref, ref_grad = value_and_grad(lambda x: reduce_(restate(x, target, ALPHA, gamma, IGNORE, wt, pre_softmax), reduction), logits.double(), cot)
            _y, yard_grad = value_and_grad(yard, logits, cot)
            got, got_grad = value_and_grad(hip, x_dev, cot)
            assert got.dtype == torch.float32 and got_grad.stride() == x_dev.stride()
            check(got, got_grad, ref, ref_grad, yard_grad, f"C{c} {h}x{w} gamma {gamma} pre {int(pre_softmax)} w {int(weighted)} {reduction}")
            ignored = (target == IGNORE)[:, None].expand_as(logits)
            assert bool((got_grad.cpu()[ignored] == 0).all())                                         # exactly 0: the logits were multiplied by 0
            assert bool((got_grad.cpu()[~ignored] != 0).any())
    assert names.count("vqseg_focal_forward_f") == 6 and names.count("vqseg_focal_backward_f") == 6


@functools.lru_cache(maxsize=None)
def golden():
    return golden_io.load("focal_ref")


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("s", range(len(lc.SHAPES)))
def test_against_the_reference_golden(s, layout, monkeypatch):
    from vq_seg_amd.loss import FocalLoss, focal_loss
    fx = golden()
    logits, target, _clean, cot = lc.inputs(s)
    x_dev = logits.to(DEV).contiguous(memory_format=torch.channels_last) if layout == "channels_last" else logits.to(DEV)
    t_dev, w, w_dev = target.to(DEV), lc.weight(), lc.weight().to(DEV)
    names = launches(monkeypatch)
    cases = [(lc.focal_key(s, g, wf, r), g, wf, r, False) for g in lc.GAMMAS for wf in (0, 1) for r in lc.REDUCTIONS]
    cases += [(lc.module_key(s, g, wf, r), g, wf, r, True) for g, r, wf in lc.MODULE_CASES]
    for key, gamma, weighted, reduction, module in cases:
        if module:
            mod = FocalLoss(3, lc.ALPHA, gamma, lc.IGNORE, reduction, w_dev if weighted else None)
            got, got_grad = value_and_grad(lambda x: mod(x, t_dev), x_dev, cot)
        else:
            got, got_grad = value_and_grad(lambda x: focal_loss(x, t_dev, lc.ALPHA, gamma, 3, lc.IGNORE, reduction, w_dev if weighted else None), x_dev, cot)
        _r, ref_grad = value_and_grad(lambda x: reduce_(restate(x, target, lc.ALPHA, gamma, lc.IGNORE, w if weighted else None, module), reduction),
                                      logits.double(), cot)
        check(got, got_grad, fx[key], ref_grad, fx[key + "_grad"], f"{key} {layout}")          # the yardstick: the reference's own gradient
    assert names.count("vqseg_focal_forward_f") == len(cases) and names.count("vqseg_focal_backward_f") == len(cases)


def test_two_calls_give_the_same_bits():
    from vq_seg_amd.loss import focal_loss
    logits, target, cot, weight = case_inputs(3, 17, 241)
    x, t, wd = logits.to(DEV), target.to(DEV), weight.to(DEV)
    for reduction in ("sum", "none"):
        a = value_and_grad(lambda v: focal_loss(v, t, ALPHA, 2, 3, IGNORE, reduction, wd), x, cot)
        b = value_and_grad(lambda v: focal_loss(v, t, ALPHA, 2, 3, IGNORE, reduction, wd), x, cot)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_gamma_between_0_and_1_stays_on_torch_ops_and_matches(monkeypatch):
    """(1 - p)^gamma has an unbounded derivative at p = 1 for 0 < gamma < 1: the kernel refuses it, the gate keeps it on torch ops"""
    from vq_seg_amd.loss import focal_loss
    from vq_seg_amd.loss.focal_loss import _focal_torch, focal_supported
    c, h, w = 3, 17, 31
    logits = synth.uniform(77, (B, c, h, w), -3.0, 3.0)
    _l, target, cot, weight = case_inputs(c, h, w)
    x = logits.to(DEV)
    assert focal_supported(x, c, 2) and focal_supported(x, c, 0) and not focal_supported(x, c, 0.5)
    assert not focal_supported(logits, c, 2) and not focal_supported(x.double(), c, 2) and not focal_supported(x, 5, 2)
    names = launches(monkeypatch)
    got, got_grad = value_and_grad(lambda v: focal_loss(v, target.to(DEV), ALPHA, 0.5, c, IGNORE, "mean", weight.to(DEV)), x, cot)
    assert not names
    ref, ref_grad = value_and_grad(lambda v: restate(v, target, ALPHA, 0.5, IGNORE, weight, False).mean(), logits.double(), cot)
    _y, yard_grad = value_and_grad(lambda v: _focal_torch(v, target, ALPHA, 0.5, c, IGNORE, "mean", weight), logits, cot)
    check(got, got_grad, ref, ref_grad, yard_grad, "gamma 0.5 (torch ops on the GPU)")
