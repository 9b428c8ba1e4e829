"""CutMix cost (profiles/cutmix.md): the box-mix kernel's achieved bandwidth on the benchmark step's three tensors, and the cfg3 CPS
step with cutmix_ratio = 0.25 next to the same step with None -- two trainers in ONE process, timed in interleaved rounds.

    python tools/bench_cutmix.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--only off|cutmix] [--out FILE]
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


def kernel_bandwidth(dev, batch, size, reps=20):
    from vq_seg_amd import _hip
    from vq_seg_amd.data import augmentations as A
    boxes = A.step_boxes(batch, size, size, 0.25, 42, 0, 0, "sample")
    cases = {"images f32 channels_last": torch.rand(batch, 3, size, size, device=dev).contiguous(memory_format=torch.channels_last),
             "scores f32 nchw": torch.rand(batch, 3, size, size, device=dev),
             "labels i64": torch.randint(0, 3, (batch, size, size), device=dev)}
    rows = {}
    for name, t in cases.items():
        out = torch.empty_like(t)
        for _ in range(3):
            _hip.box_mix(t, boxes, out=out)
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _hip.box_mix(t, boxes, out=out)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = statistics.median(times)
        nbytes = 2 * t.numel() * t.element_size()             # one read + one write per element
        rows[name] = {"bytes": nbytes, "ms_median": round(ms, 4), "ms_min": round(min(times), 4), "GB_per_s": round(nbytes / ms / 1e6, 1)}
    return rows


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    trainers = {}
    for key, ratio in (("off", None), ("cutmix", 0.25)):
        if only and key != only:
            continue
        cfg = CPSConfig(model=bench.model_cfg("cfg3"), recipe=wl["recipe"], total_iters=rounds * steps + 8, amp_dtype=torch.bfloat16, cutmix_ratio=ratio)
        trainers[key] = CPSTrainer(cfg, dev)
        for i in range(2):                                      # warm-up (k-means init, weight images, allocator)
            (l_in, l_tg), ul = batches[i % 2]
            trainers[key].step(l_in, l_tg, ul)
        torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for r in range(rounds):
        for key in [k for k in (("off", "cutmix") if r % 2 == 0 else ("cutmix", "off")) if k in trainers]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                (l_in, l_tg), ul = batches[i % 2]
                trainers[key].step(l_in, l_tg, ul)
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3 / steps)
    return {k: {"ms_per_step_rounds": [round(v, 2) for v in vs], "median": round(statistics.median(vs), 2)} for k, vs in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--only", default="", choices=["", "off", "cutmix"], help="time one of the two steps only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_bandwidth(dev, args.batch, args.size)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
    if not args.no_step and not args.only:
        off, on = res["step"]["off"]["median"], res["step"]["cutmix"]["median"]
        res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
