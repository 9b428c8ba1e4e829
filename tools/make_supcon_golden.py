"""Writes tests/golden/supcon_ref.npz: what the REFERENCE's SupConLoss (loss/contrastive_loss.py, imported through
oracle/ref_harness.install()) computes for the seeded inputs of tests/supcon_cases.py -- the loss and its autograd.grad with respect to
the features, at a feature scale where the reference's plain exp stays finite (asserted: every stored value finite, max z <= 60).
Data only; needs the reference tree, so it runs where the goldens are made, never in a test.

    python tools/make_supcon_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import supcon_cases as sc  # noqa: E402


def main():
    ref_harness.install()
    import loss as ref                                       # the reference's package
    out = {}
    mod = ref.SupConLoss(sc.TEMPERATURE)
    for k in range(len(sc.GOLDEN_CASES)):
        x, target = sc.golden_inputs(k)
        xg = x.clone().requires_grad_(True)
        y = mod(xg, target)
        (g,) = torch.autograd.grad(y, xg)
        zmax = sc.restate64(x, target)["zmax"]
        assert zmax <= 60.0, f"case {k}: max z = {zmax} (the reference's exp must stay far from float32 overflow)"
        out[f"loss_{k}"], out[f"grad_{k}"], out[f"zmax_{k}"] = y.detach().numpy(), g.numpy(), np.float64(zmax)
    assert all(np.isfinite(v).all() for v in out.values())
    out["meta"] = np.array(json.dumps({"source": "loss/contrastive_loss.py of the reference", "inputs": "tests/supcon_cases.py",
                                       "cases": [list(map(list, c[:2])) + [c[2]] for c in sc.GOLDEN_CASES], "temperature": sc.TEMPERATURE,
                                       "scale": sc.GOLDEN_SCALE}))
    path = os.path.join(ROOT, "tests", "golden", "supcon_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays", {k: float(v) for k, v in out.items() if k.startswith(("zmax", "loss"))})


if __name__ == "__main__":
    main()
