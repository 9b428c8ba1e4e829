"""Writes tests/golden/focal_ref.npz: what the REFERENCE's loss package (imported through oracle/ref_harness.install()) computes for
the seeded inputs of tests/loss_cases.py -- focal_loss for three reductions x {no weight, weight} x gamma {0, 2, 3} with ignored
pixels and one image ignored entirely, FocalLoss in module form, compute_class_weight, F.cross_entropy(weight=) and
dice_loss(weight=), each scalar with its autograd.grad with respect to the logits (reduction 'none': of sum(loss * cotangent)).
Data only; needs the reference tree, so it runs where the goldens are made, never in a test.

    python tools/make_loss_golden.py
"""
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import loss_cases as lc  # noqa: E402


def with_grad(fn, logits, cot=None):
    x = logits.clone().requires_grad_(True)
    y = fn(x)
    scalar = y if y.dim() == 0 else (y * cot).sum()
    (g,) = torch.autograd.grad(scalar, x)
    return y.detach().numpy(), g.numpy()


def main():
    ref_harness.install()
    import loss as ref                                       # the reference's package
    out = {}
    w = lc.weight()
    for s in range(len(lc.SHAPES)):
        logits, target, clean, cot = lc.inputs(s)
        for gamma in lc.GAMMAS:
            for weighted in (0, 1):
                for red in lc.REDUCTIONS:
                    key = lc.focal_key(s, gamma, weighted, red)
                    out[key], out[key + "_grad"] = with_grad(
                        lambda x: ref.focal_loss(x, target, lc.ALPHA, gamma, 3, lc.IGNORE, red, w if weighted else None), logits, cot)
        for gamma, red, weighted in lc.MODULE_CASES:
            key = lc.module_key(s, gamma, weighted, red)
            mod = ref.FocalLoss(3, lc.ALPHA, gamma, lc.IGNORE, red, w if weighted else None)
            out[key], out[key + "_grad"] = with_grad(lambda x: mod(x, target), logits, cot)
        out[f"cw_{s}"] = ref.compute_class_weight(3, clean).numpy()
        out[f"cw255_{s}"] = ref.compute_class_weight(3, target).numpy()          # bincount grows to 256 entries
        out[f"ce_{s}"], out[f"ce_{s}_grad"] = with_grad(lambda x: F.cross_entropy(x, target, weight=w, ignore_index=lc.IGNORE), logits)
        out[f"dicew_{s}"], out[f"dicew_{s}_grad"] = with_grad(
            lambda x: ref.make_loss_as_func("dice_loss")(x, target, num_classes=3, weight=w, ignore_index=lc.IGNORE), logits)
    out["cw_missing"] = ref.compute_class_weight(3, lc.missing_class_labels()).numpy()
    assert all(np.isfinite(v).all() for v in out.values())
    out["meta"] = np.array(json.dumps({"source": "loss/focal_loss.py, loss/__init__.py, loss/dice_loss.py of the reference",
                                       "inputs": "tests/loss_cases.py", "shapes": lc.SHAPES, "alpha": lc.ALPHA, "weight": lc.WEIGHT}))
    path = os.path.join(ROOT, "tests", "golden", "focal_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
