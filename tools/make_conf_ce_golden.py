"""Writes tests/golden/conf_ce_ref.npz: what the REFERENCE's conf_ce_loss and cal_unsuploss_weight
(deprecated/train_vq_pt_unet_conf_ce.py:34-113) compute for the golden cases of tests/conf_ce_cases.py -- the loss and its
autograd.grad with respect to inputs AND targets, in float32 and in float64, and the unreliable weight at two percents.
Data only.  The two functions are taken from the reference file at run time: the file is parsed with `ast`, the two function
nodes are compiled and executed in a namespace that holds torch and numpy (importing the trainer module would pull in wandb and
the datasets).  Needs the reference tree, so it runs where the goldens are made, never in a test.

    python tools/make_conf_ce_golden.py [REFERENCE_ROOT]

Where the reference has no value -- its empty negative mean is NaN (Mn == 0), and with no confident pixel and threshold_neg == 0
it returns a constant 0 without a graph -- nothing but the fact is stored (meta: "nan", "no_graph")."""
import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402  (where the reference tree lies; nothing of it is imported)
from tests import conf_ce_cases as cc  # noqa: E402

SOURCE = os.path.join("deprecated", "train_vq_pt_unet_conf_ce.py")


def reference_functions(ref_root):
    path = os.path.join(ref_root, SOURCE)
    tree = ast.parse(open(path).read(), filename=path)
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("conf_ce_loss", "cal_unsuploss_weight")]
    assert len(wanted) == 2, [n.name for n in wanted]
    ns = {"torch": torch, "np": np}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), path, "exec"), ns)
    return ns["conf_ce_loss"], ns["cal_unsuploss_weight"]


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_harness.REF_ROOT
    conf_ce_loss, cal_unsuploss_weight = reference_functions(ref_root)
    out, nan, no_graph, redrawn = {}, [], [], {}
    for name in cc.GOLDEN_CASES:
        a, b, redrawn[name] = cc.golden_inputs(name)
        thr, thrn, temp = cc.params(name)
        for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
            x, t = a.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True)
            y = conf_ce_loss(x, t, True, thr, thrn, temp)
            if not bool(torch.isfinite(y)):
                nan.append(f"{name}_{tag}")
                continue
            out[f"{name}_{tag}_loss"] = y.detach().numpy()
            if not y.requires_grad:
                no_graph.append(f"{name}_{tag}")
                continue
            gx, gt = torch.autograd.grad(y, (x, t))
            out[f"{name}_{tag}_gx"], out[f"{name}_{tag}_gt"] = gx.numpy(), gt.numpy()
    a, _b, _ = cc.golden_inputs("ref")
    for p in cc.GOLDEN_PERCENTS:
        # the call site's arguments (:225): arg-max pseudo labels of the target-side logits, nothing is 255
        uw = cal_unsuploss_weight(a, torch.argmax(a, dim=1).long().clone(), p, a.detach())
        out[f"uw_{p}"] = np.asarray(uw.numpy())
    assert all(np.isfinite(v).all() for v in out.values())
    out["meta"] = np.array(json.dumps({"source": SOURCE + ":34-113 of the reference", "inputs": "tests/conf_ce_cases.py golden_inputs",
                                       "cases": {n: list(cc.CASES[n]) for n in cc.GOLDEN_CASES}, "scale": cc.GOLDEN_SCALE, "shape": list(cc.GOLDEN_SHAPE),
                                       "nan": nan, "no_graph": no_graph, "redrawn": redrawn, "percents": list(cc.GOLDEN_PERCENTS)}))
    path = os.path.join(ROOT, "tests", "golden", "conf_ce_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays; nan:", nan, "no graph:", no_graph, "redrawn:", redrawn)
    print({k: float(v) for k, v in out.items() if k.endswith("_loss") or k.startswith("uw_")})


if __name__ == "__main__":
    main()
