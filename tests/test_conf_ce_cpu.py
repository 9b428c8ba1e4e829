"""The confidence-weighted CPS loss without a GPU: the float64 restatement of tests/conf_ce_cases.py against what the reference
computed (tests/golden/conf_ce_ref.npz), the torch-op form of loss.conf_ce_loss -- the CPU path and the GPU tests' yardstick --
against the reference's float32 values, the two deliberate deviations, the unreliable weight, the margin rule of the cases, the
configuration's validation and the flat `loss` names.

Bars.  Restatement against the reference's own float64 run: 1e-12 of the largest entry (both are float64 evaluations of one
formula; the golden logits are moderate, so the reference's `1 - softmax` keeps its digits).  Torch-op form against the reference's
float32 run: 4 float32 ulp of the largest entry -- the same operations, only the two masked means are taken as sum / count."""
import functools
import subprocess
import sys
import os

import numpy as np
import pytest
import torch

from tests import conf_ce_cases as cc, golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_SHAPES = [(3, 2, 9, 13), (3, 3, 17, 31), (3, 4, 17, 241), (3, 3, 17, 241)]      # tests/test_conf_ce_kernel_gpu.py


@functools.lru_cache(maxsize=None)
def golden():
    return golden_io.load("conf_ce_ref")


def _close(got, ref, rel, what):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    err, bar = float((got - ref).abs().max()), rel * float(ref.abs().max())
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar, what


def _ulp_close(got, ref, ulps, what):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    err, bar = float((got - ref).abs().max()), ulps * float(np.spacing(np.float32(ref.abs().max())))
    print(f"{what}: err {err:.3e} bar {bar:.3e} ({ulps} ulp)")
    assert err <= bar, what


@pytest.mark.parametrize("name", cc.GOLDEN_CASES)
def test_restatement_equals_the_references_float64_run(name):
    fx = golden()
    a, b, _ = cc.golden_inputs(name)
    loss, gx, gt = cc.restate_grads(a, b, *cc.params(name))
    if f"{name}_f64" in fx.meta["nan"]:
        assert name == "mn0" and bool(torch.isfinite(loss))            # the reference has no value here
        return
    _close(loss, fx[f"{name}_f64_loss"], 1e-12, f"{name} loss")
    if f"{name}_f64" in fx.meta["no_graph"]:
        assert name == "m0" and float(loss) == 0.0
        return
    _close(gx, fx[f"{name}_f64_gx"], 1e-12, f"{name} d/dx")
    _close(gt, fx[f"{name}_f64_gt"], 1e-12, f"{name} d/dt")
    assert float(fx[f"{name}_f64_gt"].abs().max()) > 0                 # the targets are not detached


@pytest.mark.parametrize("name", cc.GOLDEN_CASES)
def test_torch_op_form_on_the_cpu_agrees_with_the_references_float32_run(name):
    from vq_seg_amd.loss import ConfCELoss, conf_ce_loss
    fx = golden()
    a, b, _ = cc.golden_inputs(name)
    thr, thrn, temp = cc.params(name)
    x, t = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = conf_ce_loss(x, t, True, thr, thrn, temp)
    assert y.dtype == torch.float32 and y.requires_grad
    assert torch.equal(ConfCELoss(True, thr, thrn, temp)(a, b), y.detach())
    if f"{name}_f32" in fx.meta["nan"]:
        assert bool(torch.isfinite(y))
        return
    _ulp_close(y.detach(), fx[f"{name}_f32_loss"], 4, f"{name} loss")
    if f"{name}_f32" in fx.meta["no_graph"]:
        return
    gx, gt = torch.autograd.grad(y, (x, t))
    _ulp_close(gx, fx[f"{name}_f32_gx"], 4, f"{name} d/dx")
    _ulp_close(gt, fx[f"{name}_f32_gt"], 4, f"{name} d/dt")


def test_no_confident_pixel_gives_an_attached_zero_and_an_empty_negative_mask_a_finite_loss():
    from vq_seg_amd.loss import conf_ce_loss
    a, b, _ = cc.golden_inputs("m0")
    x, t = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = conf_ce_loss(x, t, True, *cc.params("m0"))
    gx, gt = torch.autograd.grad(y, (x, t))
    assert float(y.detach()) == 0.0 and y.requires_grad and not bool(gx.any()) and not bool(gt.any())
    a, b, _ = cc.golden_inputs("mn0")
    x, t = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    thr, thrn, temp = cc.params("mn0")
    y = conf_ce_loss(x, t, True, thr, thrn, temp)
    gx, gt = torch.autograd.grad(y, (x, t))
    assert bool(torch.isfinite(y)) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gt).all())
    parts = {}
    ref = cc.restate(a, b, thr, thrn, temp, parts=parts)
    assert parts["mn"] == 0 and parts["m"] > 0
    _close(y.detach(), ref, 2e-6, "Mn == 0: positive term + regulariser")


def test_detach_targets_and_conf_mask_false():
    from vq_seg_amd.loss import conf_ce_loss
    a, b, _ = cc.golden_inputs("neg")
    x, t = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = conf_ce_loss(x, t, True, *cc.params("neg"), detach_targets=True)
    gx, gt = torch.autograd.grad(y, (x, t), allow_unused=True)
    assert gt is None
    y2 = conf_ce_loss(x, t, True, *cc.params("neg"))
    assert torch.equal(y.detach(), y2.detach()) and torch.equal(gx, torch.autograd.grad(y2, x)[0])
    with pytest.raises(NotImplementedError):
        conf_ce_loss(a, b, conf_mask=False)


@pytest.mark.parametrize("percent", cc.GOLDEN_PERCENTS)
def test_unreliable_weight_equals_the_references(percent):
    from vq_seg_amd.loss import unreliable_weight
    a, _b, _ = cc.golden_inputs("ref")
    uw = unreliable_weight(a, percent)
    assert uw.dim() == 0 and uw.dtype == torch.float32
    assert torch.equal(uw, golden()[f"uw_{percent}"].reshape(()))
    assert abs(float(uw) - cc.unreliable_weight64(a, percent)) <= 1e-6 * float(uw)


def test_every_case_is_margin_clean_and_under_the_redraw_cap():
    seen = {}
    for name in cc.CASES:
        thr, thrn, temp = cc.params(name)
        built = [(shape, cc.inputs(name, shape)) for shape in GPU_SHAPES]
        if name in cc.GOLDEN_CASES:
            built.append((cc.GOLDEN_SHAPE, cc.golden_inputs(name)))
        for shape, (a, b, redrawn) in built:
            assert not bool(cc._violations(a, b, thr, thrn, temp).any()) and not bool(cc._violations(b, a, thr, thrn, temp).any())
            pixels = shape[0] * shape[2] * shape[3]
            seen[(name, shape)] = redrawn
            assert redrawn < 0.01 * pixels, (name, shape, redrawn, pixels)
            parts = {}
            cc.restate(a, b, thr, thrn, temp, parts=parts)
            if name == "m0":
                assert parts["m"] == 0
            elif name == "mn0":
                assert parts["mn"] == 0 and parts["m"] > 0
            else:
                assert 0 < parts["m"] and (thrn == 0 or 0 < parts["mn"])
            if name == "clamp":                                       # clamped elements inside the negative mask, off the arg-max
                assert float(a.abs().max()) < 12 and float(b.abs().max()) < 12
                r = torch.softmax(b.double() / temp, dim=1)
                off = torch.arange(shape[1]).view(1, -1, 1, 1) != r.argmax(dim=1, keepdim=True)
                assert int(((cc.one_minus_softmax(a.double()) < 1e-7) & (r < thrn) & off).sum()) > 0, shape
    print("redrawn pixels:", seen)


def test_config_validation():
    from vq_seg_amd.trainer import CPSConfig
    cfg = CPSConfig(model={})
    assert cfg.unsup_criterion is None
    assert (cfg.conf_ce_threshold, cfg.conf_ce_threshold_neg, cfg.conf_ce_temperature) == (0.6, 0.0, 1.0)
    assert cfg.conf_ce_unreliable_weight is True and cfg.conf_ce_detach_targets is False
    CPSConfig(model={}, unsup_criterion="conf_ce", criterion="focal_loss", class_weight="balanced")     # composes with the criteria
    with pytest.raises(ValueError):
        CPSConfig(model={}, unsup_criterion="conf_ce", recipe="v2")
    with pytest.raises(ValueError):
        CPSConfig(model={}, unsup_criterion="soft")
    with pytest.raises(ValueError):
        CPSConfig(model={}, unsup_criterion="conf_ce", conf_ce_temperature=0.0)
    with pytest.raises(ValueError):
        CPSConfig(model={}, unsup_criterion="conf_ce", conf_ce_threshold_neg=-0.1)


def test_not_in_the_label_criterion_tables():
    import vq_seg_amd.loss as L
    assert "conf_ce_loss" not in L.loss_func_dict and "conf_ce_loss" not in L.loss_dict


def test_compat_flat_loss_exposes_the_names():
    code = ("import loss, vq_seg_amd.loss as real\n"
            "assert loss.conf_ce_loss is real.conf_ce_loss and loss.ConfCELoss is real.ConfCELoss\n"
            "assert loss.unreliable_weight is real.unreliable_weight\n"
            "from loss.conf_ce_loss import conf_ce_loss\n"
            "assert conf_ce_loss is real.conf_ce_loss\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


def test_cpu_tensors_never_reach_the_library(monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss import conf_ce_loss
    a, b, _ = cc.golden_inputs("neg")
    assert not nnf.conf_ce_supported(a, b)
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *args, **kw: (names.append(name), real(name, *args, **kw))[1])
    conf_ce_loss(a, b, True, *cc.params("neg"))
    assert not names
    from vq_seg_amd._hip import HipLibraryError
    with pytest.raises(HipLibraryError, match="no CPU fallback"):
        nnf.conf_ce(a, b)                                              # below the loss package a CPU tensor is an error


def test_entry_points_refuse_bad_arguments_before_touching_a_device():
    from vq_seg_amd import _hip
    L = _hip.lib()
    nb = -(-(17 * 241) // 4096)                                        # DICE_PX_PER_BLOCK
    # per direction, image and block 3 doubles + 2 int64, per direction and image the same once more; always sized for the pair
    assert L.vqseg_conf_ce_workspace_bytes(3, 17 * 241) == 2 * 3 * (nb + 1) * 5 * 8
    assert L.vqseg_conf_ce_workspace_bytes(0, 100) == 0 and L.vqseg_conf_ce_workspace_bytes(3, 0) == 0
    fwd = lambda x, c, thrn, temp, ws, nbytes: L.vqseg_conf_ce_forward_f(x, 300, 100, 1, x, 300, 100, 1, 2, c, 100, 0.6, thrn, temp, 0,       # noqa: E731
                                                                           ws, nbytes, None, None, None)
    for args, msg in (((None, 3, 0.0, 1.0, None, 0), b"null pointer"), ((1 << 12, 5, 0.0, 1.0, None, 0), b"2..4 classes"),
                      ((1 << 12, 3, 0.0, 0.0, None, 0), b"temperature"), ((1 << 12, 3, -1.0, 1.0, None, 0), b"threshold_neg"),
                      ((1 << 12, 3, 0.0, 1.0, None, 0), b"null pointer")):
        assert fwd(*args) != 0 and msg in L.vqseg_last_error(), (args, L.vqseg_last_error())
    rc = L.vqseg_conf_ce_backward_f(1 << 12, 300, 100, 1, 1 << 12, 300, 100, 1, 2, 3, 100, 0.6, 0.0, 1.0, 1, 1, 1 << 12, 1 << 12, 1 << 12, None, None)
    assert rc != 0 and b"target-side gradient" in L.vqseg_last_error()        # only a single call with detached targets may leave it out
