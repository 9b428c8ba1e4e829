"""Focal loss cost (profiles/focal_loss.md): the fused focal forward + backward at the step's logit shape (64 x 3 x 512 x 512: labelled +
unlabelled halves of a batch-32 step) in microseconds and GB/s, the Dice + CE pass (vqseg_dice_ce_sums_*) at the same shape -- both
are one read of logits and targets forward, one more read plus one write of the gradient backward --, the torch-op formulation on
the GPU, the class-weight count, and the cfg3 CPS step with class_weight="balanced" next to the plain step -- two trainers in ONE
process, timed in interleaved rounds.

    python tools/bench_focal.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--only off|balanced|focal] [--out FILE]
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


def _time(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times), min(times)


def kernel_rates(dev, batch, size, reps=20):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss.focal_loss import _focal_torch
    c, hw = 3, size * size
    target = torch.randint(0, 3, (batch, size, size), device=dev)
    target[torch.rand(batch, size, size, device=dev) < 0.2] = 255
    weight = torch.tensor([0.5, 0.8, 1.0], device=dev)
    fwd_bytes = batch * hw * (c * 4 + 8)                      # logits + int64 targets
    bwd_bytes = fwd_bytes + batch * hw * c * 4               # ... again, + the gradient
    rows = {}
    for layout in ("nchw", "channels_last"):
        x = torch.randn(batch, c, size, size, device=dev)
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        one = torch.ones((), device=dev)
        passes = {
            "focal gamma 2 weighted": lambda: nnf.focal(x, target, 0.25, 2.0, 255, "mean", weight, False),
            "focal gamma 2 weighted module form": lambda: nnf.focal(x, target, 0.25, 2.0, 255, "mean", weight, True),
            "focal gamma 2.5 (powf)": lambda: nnf.focal(x, target, 0.25, 2.5, 255, "mean", None, False),
            "weighted ce sums": lambda: nnf.wce_sums(x, target, weight, 255).sum(),
            "dice + ce sums": lambda: sum(t.sum() for t in nnf.dice_ce_sums(x, target, 255)),
            "torch ops focal (module form)": lambda: _focal_torch(torch.softmax(x, 1), target, 0.25, 2.0, 3, 255, "mean", weight),
        }
        for name, fwd in passes.items():
            with torch.no_grad():
                f_med, f_min = _time(fwd, reps)
            y = fwd()

            def bwd():
                x.grad = None
                y.backward(one, retain_graph=True)

            b_med, b_min = _time(bwd, reps)
            rows[f"{name} {layout}"] = {"forward_us": round(f_med, 1), "forward_us_min": round(f_min, 1), "backward_us": round(b_med, 1),
                                        "backward_us_min": round(b_min, 1), "forward_GB_per_s": round(fwd_bytes / f_med / 1e3, 1),
                                        "backward_GB_per_s": round(bwd_bytes / b_med / 1e3, 1)}
    lab = target[: batch // 2]
    med, mn = _time(lambda: nnf.class_weight(3, lab), reps)
    rows["class weight count (labelled half)"] = {"us": round(med, 1), "us_min": round(mn, 1), "GB_per_s": round(lab.numel() * 8 / med / 1e3, 1)}
    return {"shape": [batch, c, size, size], "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
            "note": "forward/backward times of the torch-op and sums rows include their scalar epilogues; every row is events around the call", "rows": rows}


ARMS = {"off": {}, "balanced": dict(class_weight="balanced"), "focal": dict(criterion="focal_loss", class_weight="balanced")}


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    keys = [only] if only else ["off", "balanced"]
    trainers = {}
    for key in keys:
        cfg = CPSConfig(model=bench.model_cfg("cfg3"), recipe=wl["recipe"], total_iters=rounds * steps + 8, amp_dtype=torch.bfloat16, **ARMS[key])
        trainers[key] = CPSTrainer(cfg, dev)
        for i in range(2):                                      # warm-up (k-means init, weight images, allocator)
            (l_in, l_tg), ul = batches[i % 2]
            trainers[key].step(l_in, l_tg, ul)
        torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--only", default="", choices=[""] + sorted(ARMS), help="time one step arm only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_rates(dev, args.batch, args.size)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
        if not args.only:
            off, on = res["step"]["off"]["median"], res["step"]["balanced"]["median"]
            res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
