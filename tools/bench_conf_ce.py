"""Confidence-weighted CPS loss cost (profiles/conf_ce.md): the fused forward and backward, single and pair, at the unlabelled
half of a batch-32 step (32 x 3 x 512 x 512 input logits and as many target logits) in microseconds and GB/s of algorithmic bytes,
the torch-op form of the same loss (loss.conf_ce_loss's fallback) on the GPU in the same run, the unreliable weight, and the cfg3 CPS
step with unsup_criterion="conf_ce" next to the plain step -- two trainers in ONE process, timed in interleaved rounds.

Algorithmic bytes: the forward reads both logit tensors once (2 * 4 * C bytes per pixel), the backward reads them again and writes
both gradients (as much again); single or pair, detached targets write one gradient less.

    python tools/bench_conf_ce.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--only off|conf_ce] [--out FILE]
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

PARAMS = {"reference call (0.6, 0, 1)": (0.6, 0.0, 1.0), "negative term (0.6, 0.1, 1)": (0.6, 0.1, 1.0), "temperature (0.6, 0.1, 2)": (0.6, 0.1, 2.0)}


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
    from vq_seg_amd.loss.conf_ce_loss import _conf_ce_torch, unreliable_weight
    c, hw = 3, size * size
    fwd_bytes = batch * hw * 2 * c * 4                          # both logit tensors
    bwd_bytes = 2 * fwd_bytes                                   # ... again, + both gradients
    rows = {}
    one = torch.ones((), device=dev)
    for layout in ("nchw", "channels_last"):
        a, b = torch.randn(batch, c, size, size, device=dev) * 3, torch.randn(batch, c, size, size, device=dev) * 3
        if layout == "channels_last":
            a, b = a.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last)
        a.requires_grad_(True), b.requires_grad_(True)
        for pname, par in PARAMS.items():
            passes = {
                "fused single": lambda: nnf.conf_ce(a, b, *par),
                "fused pair": lambda: sum(nnf.conf_ce_pair(a, b, *par)),
                "torch ops single": lambda: _conf_ce_torch(a, b, *par),
                "torch ops both directions": lambda: _conf_ce_torch(a, b, *par) + _conf_ce_torch(b, a, *par),
            }
            for name, fwd in passes.items():
                with torch.no_grad():
                    f_med, f_min = _time(fwd, reps)
                y = fwd()

                def bwd():
                    a.grad = b.grad = None
                    y.backward(one, retain_graph=True)

                b_med, b_min = _time(bwd, reps)
                rows[f"{name}, {pname}, {layout}"] = {"forward_us": round(f_med, 1), "forward_us_min": round(f_min, 1), "backward_us": round(b_med, 1),
                                                      "backward_us_min": round(b_min, 1), "forward_GB_per_s": round(fwd_bytes / f_med / 1e3, 1),
                                                      "backward_GB_per_s": round(bwd_bytes / b_med / 1e3, 1)}
                del y
        with torch.no_grad():
            med, mn = _time(lambda: unreliable_weight(b, 84.0), reps)
        rows[f"unreliable weight, {layout}"] = {"us": round(med, 1), "us_min": round(mn, 1)}
    return {"shape": [batch, c, size, size], "forward_bytes": fwd_bytes, "backward_bytes": bwd_bytes,
            "note": "events around the call: the pair rows include the sum of the two scalars, the torch-op rows every one of their kernels; "
                    "GB/s are the algorithmic bytes of ONE fused pass over the time, so the torch-op rows show the same bytes over their longer time",
            "rows": rows}


ARMS = {"off": {}, "conf_ce": dict(unsup_criterion="conf_ce"), "conf_ce_neg": dict(unsup_criterion="conf_ce", conf_ce_threshold_neg=0.1)}


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    keys = [only] if only else ["off", "conf_ce"]
    trainers = {}
    for key in keys:
        cfg = CPSConfig(model=bench.model_cfg("cfg3"), recipe="v1", total_iters=rounds * steps + 8, amp_dtype=torch.bfloat16, **ARMS[key])
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
    ap.add_argument("--batch", type=int, default=32)
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
            off, on = res["step"]["off"]["median"], res["step"]["conf_ce"]["median"]
            res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
