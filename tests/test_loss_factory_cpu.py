"""The loss factory of the reference (loss/__init__.py:5-33) on a box without a GPU: make_loss / make_loss_as_func resolve every
name, the torch-op forms of focal_loss / FocalLoss / compute_class_weight reproduce what the reference computed
(tests/golden/focal_ref.npz, tools/make_loss_golden.py), the flat `loss` package binds, the new entry points are declared, their
wrappers refuse wrong types and sizes before any device is touched, and recipe v2 refuses the v1-only switches."""
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import golden_io, loss_cases as lc
from vq_seg_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["vqseg_focal_workspace_bytes", "vqseg_focal_forward_f", "vqseg_focal_backward_f", "vqseg_wce_sums_forward_f",
               "vqseg_wce_sums_backward_f", "vqseg_class_weight_f"]


def test_make_loss_returns_a_focal_loss():
    from vq_seg_amd.loss import FocalLoss, make_loss
    crit = make_loss("focal_loss", 3, ignore_index=255)
    assert isinstance(crit, FocalLoss)
    assert (crit.num_classes, crit.alpha, crit.gamma, crit.ignore_index, crit.reduction, crit.weight) == (3, 0.25, 2, 255, "mean", None)
    with pytest.raises(KeyError):
        make_loss("no_such_loss", 3)


def test_make_loss_as_func_resolves_all_four_names():
    from vq_seg_amd import loss
    assert sorted(loss.loss_func_dict) == sorted(loss.loss_dict) == ["cross_entropy", "dice_loss", "focal_loss", "nll_loss"]
    assert loss.make_loss_as_func("dice_loss") is loss.dice_loss and loss.make_loss_as_func("focal_loss") is loss.focal_loss
    assert loss.make_loss_as_func("nll_loss") is F.nll_loss
    ce = loss.make_loss_as_func("cross_entropy")
    logits, target, _clean, _cot = lc.inputs(0)
    want = F.cross_entropy(logits, target, weight=lc.weight(), ignore_index=lc.IGNORE)
    assert torch.equal(ce(logits, target, weight=lc.weight(), ignore_index=lc.IGNORE), want)      # CPU: F.cross_entropy itself
    assert torch.equal(ce(logits, target, ignore_index=lc.IGNORE), F.cross_entropy(logits, target, ignore_index=lc.IGNORE))


def test_compute_class_weight_on_cpu_equals_the_golden():
    from vq_seg_amd.loss import compute_class_weight
    fx = golden_io.load("focal_ref")
    for s in range(len(lc.SHAPES)):
        _logits, target, clean, _cot = lc.inputs(s)
        assert torch.equal(compute_class_weight(3, clean), fx[f"cw_{s}"])
        assert torch.equal(compute_class_weight(3, target), fx[f"cw255_{s}"])             # bincount's longer vector, as the reference
    got = compute_class_weight(3, lc.missing_class_labels())
    assert torch.equal(got, fx["cw_missing"]) and float(got[1]) == 1.0


def _value_and_grad(fn, logits, cot):
    x = logits.clone().requires_grad_(True)
    y = fn(x)
    (g,) = torch.autograd.grad(y if y.dim() == 0 else (y * cot).sum(), x)
    return y.detach(), g


def test_cpu_focal_loss_equals_the_golden():
    """the torch-op form IS the reference's arithmetic: the same operations in the same order, so the same bits"""
    from vq_seg_amd.loss import FocalLoss, focal_loss
    fx = golden_io.load("focal_ref")
    w = lc.weight()
    for s in range(len(lc.SHAPES)):
        logits, target, _clean, cot = lc.inputs(s)
        for gamma in lc.GAMMAS:
            for weighted in (0, 1):
                for red in lc.REDUCTIONS:
                    key = lc.focal_key(s, gamma, weighted, red)
                    y, g = _value_and_grad(lambda x: focal_loss(x, target, lc.ALPHA, gamma, 3, lc.IGNORE, red, w if weighted else None), logits, cot)
                    assert torch.equal(y, fx[key]), key
                    assert torch.equal(g, fx[key + "_grad"]), key
        for gamma, red, weighted in lc.MODULE_CASES:
            key = lc.module_key(s, gamma, weighted, red)
            mod = FocalLoss(3, lc.ALPHA, gamma, lc.IGNORE, red, w if weighted else None)
            y, g = _value_and_grad(lambda x: mod(x, target), logits, cot)
            assert torch.equal(y, fx[key]), key
            assert torch.equal(g, fx[key + "_grad"]), key
    with pytest.raises(NotImplementedError):
        focal_loss(logits, target, lc.ALPHA, 2, 3, lc.IGNORE, "median")


def test_an_ignored_pixel_is_a_zero_logit_class_0_pixel():
    """the kept quirk (focal_loss.py:12-14), in closed form: alpha * w[0] * (1 - 1/C)^gamma * log C per ignored pixel"""
    from vq_seg_amd.loss import focal_loss
    logits = lc.inputs(0)[0][:1]
    target = torch.full((1, 9, 13), lc.IGNORE)
    got = focal_loss(logits, target, lc.ALPHA, 2, 3, lc.IGNORE, "mean", lc.weight())
    assert abs(float(got) - lc.ALPHA * 0.5 * (2 / 3) ** 2 * np.log(3)) < 1e-7


SCRIPT = textwrap.dedent('''
    import json, sys
    sys.path.insert(0, sys.argv[1])                 # <repo>/compat
    import torch
    from loss import make_loss_as_func, compute_class_weight          # deprecated/train_vq_pt_unet_balncedweightedloss.py:26
    from loss import make_loss, FocalLoss, focal_loss, loss_dict, loss_func_dict
    from loss.focal_loss import FocalLoss as F2
    import vq_seg_amd.loss
    criterion = make_loss_as_func("dice_loss")
    y = torch.tensor([[0, 0, 1, 2]])
    w = compute_class_weight(3, y)
    pred = torch.zeros(1, 3, 1, 4)
    print(json.dumps({"same": FocalLoss is vq_seg_amd.loss.FocalLoss and F2 is FocalLoss and focal_loss is vq_seg_amd.loss.focal_loss,
                      "focal": type(make_loss("focal_loss", 3, ignore_index=255)).__name__, "names": sorted(loss_func_dict),
                      "w": w.tolist(), "loss": float(criterion(pred, y.reshape(1, 1, 4), weight=w))}))
''')


def test_flat_loss_package_exposes_the_new_names(tmp_path):
    script = tmp_path / "balanced_head.py"
    script.write_text(SCRIPT)
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "compat")], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["same"] is True and out["focal"] == "FocalLoss"
    assert out["names"] == ["cross_entropy", "dice_loss", "focal_loss", "nll_loss"]
    assert out["w"] == [0.5, 0.75, 0.75] and np.isfinite(out["loss"])


def test_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vqseg.h")).read(), flags=re.S)
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} is not declared in include/vqseg.h"
        assert name in _hip.SYMBOLS and hasattr(L, name)
    # argument validation is host code
    assert L.vqseg_focal_workspace_bytes(2, 4097) == 2 * 2 * 2 * 8 and L.vqseg_focal_workspace_bytes(0, 16) == 0
    one = 1
    assert L.vqseg_focal_forward_f(one, 48, 16, 1, one, 1, 5, 16, 255, None, 0.25, 2.0, 0, one, 64, one, one, None, None) == -1
    assert b"2..4 classes" in L.vqseg_last_error()
    assert L.vqseg_focal_forward_f(one, 48, 16, 1, one, 1, 3, 16, 255, None, 0.25, 0.5, 0, one, 64, one, one, None, None) == -1
    assert b"gamma must be 0 or >= 1" in L.vqseg_last_error()
    assert L.vqseg_focal_forward_f(one, 48, 16, 1, one, 1, 3, 16, 255, None, 0.25, 2.0, 0, one, 8, one, one, None, None) == -2
    assert b"workspace too small" in L.vqseg_last_error()
    assert L.vqseg_focal_backward_f(one, 48, 16, 1, one, 1, 3, 16, 255, None, 0.25, 2.0, 0, one, 1.0, one, one, None) == -1
    assert b"exactly one" in L.vqseg_last_error()
    assert L.vqseg_wce_sums_forward_f(one, 48, 16, 1, one, 1, 3, 16, 255, None, one, 64, one, None) == -1
    assert L.vqseg_class_weight_f(one, 16, 257, one, one, None) == -1 and b"1..256 classes" in L.vqseg_last_error()
    assert L.vqseg_class_weight_f(one, 0, 3, one, one, None) == -1


WRONG = [
    ("focal bf16 logits", lambda nnf: nnf.focal(torch.zeros(1, 3, 4, 4, dtype=torch.bfloat16), torch.zeros(1, 4, 4, dtype=torch.int64), 0.25, 2, 255),
     "logits: expected a float32"),
    ("focal weight size", lambda nnf: nnf.focal(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 0.25, 2, 255, weight=torch.ones(4)),
     "class weights: the sizes passed along need 3"),
    ("focal target size", lambda nnf: nnf.focal(torch.zeros(2, 3, 4, 4), torch.zeros(1, 4, 6, dtype=torch.int64), 0.25, 2, 255),
     "shape"),
    ("focal reduction", lambda nnf: nnf.focal(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 0.25, 2, 255, "median"),
     "Invalid reduction"),
    ("focal cpu", lambda nnf: nnf.focal(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 0.25, 2, 255), "no CPU fallback"),
    ("wce f64 logits", lambda nnf: nnf.wce_sums(torch.zeros(1, 3, 4, 4, dtype=torch.float64), torch.zeros(1, 4, 4, dtype=torch.int64), torch.ones(3), 255),
     "logits: expected a float32"),
    ("wce weight size", lambda nnf: nnf.wce_sums(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), torch.ones(2), 255),
     "class weights: the sizes passed along need 3"),
    ("wce no weight", lambda nnf: nnf.wce_sums(torch.zeros(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), None, 255), "class weights: expected a tensor"),
    ("class_weight cpu", lambda nnf: nnf.class_weight(3, torch.zeros(8, dtype=torch.int64)), "no CPU fallback"),
]


@pytest.mark.parametrize("what,call,msg", WRONG, ids=[w[0] for w in WRONG])
def test_new_wrappers_refuse_wrong_types_and_sizes_before_touching_a_device(what, call, msg):
    from vq_seg_amd import nnf
    with pytest.raises((_hip.HipLibraryError, RuntimeError, NotImplementedError), match=msg):
        call(nnf)


def test_recipe_v2_refuses_the_v1_only_switches():
    from vq_seg_amd.trainer import CPSConfig
    with pytest.raises(ValueError, match="recipe 'v1'"):
        CPSConfig(model={}, recipe="v2", class_weight="balanced")
    with pytest.raises(ValueError, match="recipe 'v1'"):
        CPSConfig(model={}, recipe="v2", class_weight=[0.5, 0.8, 1.0])
    with pytest.raises(ValueError, match="recipe 'v1'"):
        CPSConfig(model={}, recipe="v2", criterion="focal_loss")
    with pytest.raises(ValueError, match="balanced"):
        CPSConfig(model={}, class_weight="inverse")
    with pytest.raises(ValueError, match="one weight per class"):
        CPSConfig(model={}, class_weight=[1.0, 2.0])
    cfg = CPSConfig(model={})
    assert (cfg.criterion, cfg.class_weight, cfg.focal_alpha, cfg.focal_gamma) == ("dice_loss", None, 0.25, 2.0)
    assert CPSConfig(model={}, recipe="v2").recipe == "v2"
    assert CPSConfig(model={}, criterion="focal_loss", class_weight="balanced", focal_gamma=3.0).focal_gamma == 3.0
