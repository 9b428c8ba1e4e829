"""Easy-augmentation cost (profiles/easy_aug.md): the affine-warp kernel's time and achieved bandwidth on the benchmark step's
tensors, and the cfg3 CPS step with easy_aug = "similarity" (alone, and together with cutmix_ratio = 0.25) next to the same step
without it -- all trainers in ONE process, timed in interleaved rounds.

    python tools/bench_easy_aug.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--only KEY] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"off": dict(), "easy": dict(easy_aug="similarity"), "cutmix": dict(cutmix_ratio=0.25), "easy+cutmix": dict(easy_aug="similarity", cutmix_ratio=0.25)}


def kernel_times(dev, batch, size, reps=20):
    """HIP-event time per launch; bytes = one read + one write per element (what the warp must move; re-reads of a rotated
    footprint that miss the caches come on top and show as a lower rate)"""
    from vq_seg_amd import _hip
    from vq_seg_amd.data import augmentations as A
    generic = A.similarity_matrices([3] * batch, [17.3] * batch)
    per_sample = A.similarity_matrices(*A.step_transforms(batch, 42, 0, 0, "sample"))
    flip = A.similarity_matrices([1] * batch, [0.0] * batch)
    img = torch.rand(batch, 3, size, size, device=dev)
    tensors = {"f32 nchw": img, "f32 channels_last": img.contiguous(memory_format=torch.channels_last)}
    cases = {}
    for lname, t in tensors.items():
        cases[f"bilinear 17.3 deg, {lname}"] = (t, generic, "bilinear")
        cases[f"bilinear per-sample draws, {lname}"] = (t, per_sample, "bilinear")
        cases[f"bilinear flip, {lname}"] = (t, flip, "bilinear")
    cases["nearest 17.3 deg, labels i64"] = (torch.randint(0, 3, (batch, size, size), device=dev), generic, "nearest")
    rows = {}
    for name, (t, mats, mode) in cases.items():
        out = torch.empty_like(t)
        for _ in range(3):
            _hip.affine_warp(t, mats, mode=mode, out=out)
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _hip.affine_warp(t, mats, mode=mode, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        nbytes = 2 * t.numel() * t.element_size()
        rows[name] = {"bytes": nbytes, "us_median": round(ms * 1e3, 1), "us_min": round(min(times) * 1e3, 1), "GB_per_s": round(nbytes / ms / 1e6, 1)}
    return rows


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    trainers = {}
    for key, kw in STEPS.items():
        if only and key != only:
            continue
        cfg = CPSConfig(model=bench.model_cfg("cfg3"), recipe=wl["recipe"], total_iters=rounds * steps + 8, amp_dtype=torch.bfloat16, **kw)
        trainers[key] = CPSTrainer(cfg, dev)
        for i in range(2):                                      # warm-up (k-means init, weight images, allocator)
            (l_in, l_tg), ul = batches[i % 2]
            trainers[key].step(l_in, l_tg, ul)
        torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    keys = list(trainers)
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                (l_in, l_tg), ul = batches[i % 2]
                trainers[key].step(l_in, l_tg, ul)
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: {"ms_per_step_rounds": [round(v, 2) for v in vs], "median": round(statistics.median(vs), 2),
                "spread": round(max(vs) - min(vs), 2)} for k, vs in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--only", default="", choices=[""] + list(STEPS), help="time one of the steps only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_easy_aug: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_times(dev, args.batch, args.size)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
    if not args.no_step and not args.only:
        st = res["step"]
        for on, off in (("easy", "off"), ("easy+cutmix", "cutmix")):
            d = st[on]["median"] - st[off]["median"]
            st[f"cost_ms {on} vs {off}"], st[f"cost_percent {on} vs {off}"] = round(d, 2), round(100 * d / st[off]["median"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
