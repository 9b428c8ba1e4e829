"""Fingerprints of the CPS step with its features on, for "nothing moved" checks of trainer refactors (bench.py runs the plain step only).

    python tools/step_fingerprint.py OUT_DIR              two steps per named configuration -> OUT_DIR/<name>.npz
    python tools/step_fingerprint.py --compare A B        every array of every file of A against B: equal / DIFFERENT / missing

Each file holds every returned scalar and the masks / clean-frame scores (`aux`) of both steps, and the fp64 sum of every parameter
and buffer after the second.  Only the trainer's public surface is used, so the same file runs against an older tree
(`--tree DIR`: import the package from there).  Run the older tree twice first: what it does not reproduce itself cannot be compared.
"""
import argparse
import os
import sys

import numpy as np

CONFIGS = {
    "v1_bf16": dict(),
    "v2_bf16": dict(recipe="v2"),
    "v1_fp32": dict(amp=False),
    "one_stream": dict(two_streams=False),
    "cutmix_batch": dict(cutmix_ratio=0.25, cutmix_boxes="batch"),
    "cutmix_sample": dict(cutmix_ratio=0.25, cutmix_boxes="sample"),
    "easy_sample_cutmix": dict(easy_aug="similarity", easy_aug_per="sample", cutmix_ratio=0.25),
    "ema_teacher": dict(ema_decay=0.99, teacher_pseudo_labels=True),
    "focal": dict(criterion="focal_loss"),
    "balanced": dict(class_weight="balanced"),
    "fixed_weight_ce": dict(class_weight=(0.5, 1.0, 2.0), criterion="cross_entropy"),
    "wgrad_side": dict(wgrad_side_stream=True),
}


def fingerprint(name, kw, dev):
    import torch
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    kw = dict(kw)
    recipe, amp = kw.pop("recipe", "v1"), kw.pop("amp", True)
    model = {"name": "vqreptunet1x1" if recipe == "v1" else "vqreptunet1x1v2",
             "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                        "vq_cfg": {"num_embeddings": [0, 0, 32, 32, 32], "distance": "euclidean", "kmeans_init": True},
                        "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}
    torch.manual_seed(0)
    tr = CPSTrainer(CPSConfig(model=model, recipe=recipe, total_iters=10, amp_dtype=torch.bfloat16 if amp else None, keep_aux=True, seed=3, **kw), dev)
    data = SyntheticCropWeed(64, 2, dev, seed=5)
    out = {}
    for s in range(2):
        (l_in, l_tg), ul_in = data.labelled(), data.unlabelled()
        res = tr.step(l_in, l_tg, ul_in, epoch_frac=0.25 * s)
        torch.cuda.synchronize()
        for k, v in res.items():
            out[f"step{s}_{k}"] = v.detach().double().cpu().numpy()
        for k in ("mask_1", "mask_2", "score_1", "score_2"):
            out[f"step{s}_{k}"] = tr.aux[k].detach().cpu().numpy()
    for i, m in enumerate(tr.models):
        for kind, named in (("param", m.named_parameters()), ("buffer", m.named_buffers())):
            for k, t in named:
                out[f"{kind}_{i + 1}_{k}"] = t.detach().double().sum().cpu().numpy()
    return out


def compare(a, b):
    bad = 0
    for f in sorted(os.listdir(a)):
        if not f.endswith(".npz"):
            continue
        if not os.path.exists(os.path.join(b, f)):
            print(f"{f}: missing in {b}")
            bad += 1
            continue
        za, zb = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        diff = [k for k in za.files if k not in zb.files or za[k].shape != zb[k].shape or not np.array_equal(za[k], zb[k], equal_nan=True)]
        diff += [k for k in zb.files if k not in za.files]
        finite = all(np.isfinite(z[k]).all() for z in (za, zb) for k in z.files)
        print(f"{f}: {len(za.files)} arrays, {len(za.files) - len(diff)} equal, finite={finite}" + (f", DIFFERENT: {' '.join(diff)}" if diff else ""))
        bad += bool(diff)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="import vq_seg_amd from this tree")
    ap.add_argument("--only", default="", help="comma-separated configuration names")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(1 if compare(*args.compare) else 0)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("step_fingerprint: needs a GPU")
    os.makedirs(args.out, exist_ok=True)
    for name, kw in CONFIGS.items():
        if args.only and name not in args.only.split(","):
            continue
        np.savez(os.path.join(args.out, name + ".npz"), **fingerprint(name, kw, torch.device("cuda:0")))
        print(name, "written", flush=True)


if __name__ == "__main__":
    main()
