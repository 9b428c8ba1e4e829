"""compute_class_weight on the device (vqseg_class_weight_f), the class-weighted cross-entropy sums (vqseg_wce_sums_*) and
dice_loss(weight=device tensor): counts and weights exact against the CPU path and the reference's golden; the weighted
cross-entropy against F.cross_entropy(weight=) in fp64 under the bars of tests/test_focal_gpu.py (forward 2e-6 relative; gradient
within 4x the error of torch's own float32 F.cross_entropy + one float32 ulp of the largest gradient entry)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import golden_io, loss_cases as lc, synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _labels(n, seed, with_255=False, missing=False):
    lab = synth.labels(seed, (n,), 2) * 2 if missing else synth.labels(seed, (n,), 3)
    if with_255:
        lab = torch.where(synth.uniform(seed + 1, (n,)) < 0.25, torch.full_like(lab, 255), lab)
    return lab


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
@pytest.mark.parametrize("kind", ["plain", "missing", "with255"])
def test_counts_and_weights_equal_the_cpu_path(n, kind):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import compute_class_weight
    lab = _labels(n, 900 + n % 97, with_255=kind == "with255", missing=kind == "missing")
    weight, counts = nnf.class_weight(3, lab.to(DEV))
    assert weight.is_cuda and weight.dtype == torch.float32 and weight.shape == (3,) and counts.dtype == torch.int64
    want_counts = torch.bincount(lab, minlength=3)
    assert counts.cpu().tolist() == want_counts[:3].tolist() + [int(want_counts.sum())]
    cpu = compute_class_weight(3, lab)                      # the reference's two lines (a longer vector when 255 occurs)
    got = compute_class_weight(3, lab.to(DEV))
    assert got.is_cuda and torch.equal(got.cpu(), cpu[:3]) and torch.equal(got, weight)
    if kind == "missing" and n > 1:
        assert float(got[1]) == 1.0


def test_class_weight_equals_the_golden_and_takes_any_label_shape_and_class_count():
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import compute_class_weight
    fx = golden_io.load("focal_ref")
    for s in range(len(lc.SHAPES)):
        _logits, target, clean, _cot = lc.inputs(s)
        assert torch.equal(compute_class_weight(3, clean.to(DEV)).cpu(), fx[f"cw_{s}"])
        assert torch.equal(compute_class_weight(3, target.to(DEV)).cpu(), fx[f"cw255_{s}"][:3])
    assert torch.equal(compute_class_weight(3, lc.missing_class_labels().to(DEV)).cpu(), fx["cw_missing"])
    lab = synth.labels(31, (3, 40, 50), 9)                  # classes beyond the four counted in registers; a uint8 mask as the loader makes
    weight, counts = nnf.class_weight(9, lab.to(DEV).to(torch.uint8))
    assert counts.cpu().tolist() == torch.bincount(lab.flatten(), minlength=9).tolist() + [lab.numel()]
    assert torch.equal(weight.cpu(), compute_class_weight(9, lab))
    weight2, counts2 = nnf.class_weight(2, lab.to(DEV))     # labels >= num_classes count in the total only
    assert counts2.cpu().tolist() == torch.bincount(lab.flatten())[:2].tolist() + [lab.numel()]


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("c,h,w", [(2, 9, 13), (3, 17, 31), (4, 17, 241)])
def test_weighted_cross_entropy_sums(c, h, w, layout, monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import cross_entropy
    b, seed = 3, 2000 * c + h
    logits = synth.uniform(seed, (b, c, h, w), -8.0, 8.0)
    target = synth.labels(seed + 1, (b, h, w), c)
    target[0][synth.uniform(seed + 2, (h, w)) < 0.2] = 255
    target[1] = 255
    weight = synth.uniform(seed + 3, (c,), 0.3, 1.0)
    x = (logits.to(DEV).contiguous(memory_format=torch.channels_last) if layout == "channels_last" else logits.to(DEV)).requires_grad_(True)
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    got = cross_entropy(x, target.to(DEV), weight=weight.to(DEV), ignore_index=255)
    (got_grad,) = torch.autograd.grad(got, x)
    assert names == ["vqseg_wce_sums_forward_f", "vqseg_wce_sums_backward_f"] and got_grad.stride() == x.stride()
    x64 = logits.double().requires_grad_(True)
    ref = F.cross_entropy(x64, target, weight=weight.double(), ignore_index=255)
    (ref_grad,) = torch.autograd.grad(ref, x64)
    x32 = logits.clone().requires_grad_(True)
    (yard_grad,) = torch.autograd.grad(F.cross_entropy(x32, target, weight=weight, ignore_index=255), x32)
    fwd_err, k_err = abs(float(got.detach()) - float(ref.detach())), float((got_grad.cpu().double() - ref_grad).abs().max())
    y_err = float((yard_grad.double() - ref_grad).abs().max())
    bar = 4 * y_err + float(np.spacing(np.float32(ref_grad.abs().max())))
    print(f"C{c} {h}x{w} {layout}: forward err {fwd_err:.3e} (bar {2e-6 * abs(float(ref.detach())):.3e}); gradient err kernel {k_err:.3e}, "
          f"F.cross_entropy float32 {y_err:.3e}, bar {bar:.3e}")
    assert fwd_err <= 2e-6 * abs(float(ref.detach()))
    assert k_err <= bar
    assert bool((got_grad.cpu()[(target == 255)[:, None].expand_as(logits)] == 0).all())
    # the sums themselves: ce[b] = (sum of w[t] nll, sum of w[t]) over kept pixels; an ignored image contributes (0, 0)
    ce = nnf.wce_sums(x.detach(), target.to(DEV), weight.to(DEV), 255).cpu().double()
    keep = target != 255
    wt = weight.double()[target.clamp(max=c - 1)] * keep
    nll = F.cross_entropy(logits.double(), target.clamp(max=c - 1), reduction="none")
    assert torch.allclose(ce[:, 1], wt.sum(dim=(1, 2)), rtol=2e-6, atol=0) and torch.allclose(ce[:, 0], (wt * nll).sum(dim=(1, 2)), rtol=2e-6, atol=0)
    assert ce[1].tolist() == [0.0, 0.0]


def test_golden_weighted_cross_entropy_and_dice():
    """values against what the reference computed; the gradients are held to fp64 above and, for Dice, in tests/test_loss_gpu.py"""
    from vq_seg_amd.loss import dice_loss, make_loss_as_func
    fx = golden_io.load("focal_ref")
    w = lc.weight().to(DEV)
    for s in range(len(lc.SHAPES)):
        logits, target, _clean, _cot = lc.inputs(s)
        for layout in ("nchw", "channels_last"):
            x = (logits.to(DEV).contiguous(memory_format=torch.channels_last) if layout == "channels_last" else logits.to(DEV)).requires_grad_(True)
            ce = make_loss_as_func("cross_entropy")(x, target.to(DEV), weight=w, ignore_index=lc.IGNORE)
            assert abs(float(ce) - float(fx[f"ce_{s}"])) <= 2e-6 * abs(float(fx[f"ce_{s}"]))
            d = dice_loss(x, target.to(DEV), num_classes=3, weight=w, ignore_index=lc.IGNORE)      # a device weight: stays there
            assert d.is_cuda and abs(float(d) - float(fx[f"dicew_{s}"])) <= 2e-6 * max(1.0, abs(float(fx[f"dicew_{s}"])))   # the Dice bar of test_loss_gpu.py
