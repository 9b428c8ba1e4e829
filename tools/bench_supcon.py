"""Supervised contrastive loss cost (profiles/supcon.md): the fused forward and backward (vqseg_supcon_*) in microseconds at the decoder
output shapes (HW, C) = (256 x 256, 32), (128 x 128, 32), (96 x 96, 32), float32 and bfloat16 rows; at 96 x 96 the chunked torch-op form
(loss.contrastive_loss.supcon_torch) next to it; and the cfg3 CPS step with sup_con_loss_weight = 0.5 next to the plain step -- two trainers
in ONE process, timed in interleaved rounds.  There is no pass / fail time: the numbers are what the profile is for.

    python tools/bench_supcon.py [--rounds 3] [--steps 2] [--no-step] [--no-kernel] [--only off|supcon] [--out FILE]
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

SIDES = (256, 128, 96)
C, TEMPERATURE = 32, 0.04


def _time(fn, reps, warm=2):
    for _ in range(warm):
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


def kernel_times(dev, reps=5):
    from vq_seg_amd import nnf
    from vq_seg_amd.loss.contrastive_loss import supcon_torch
    gen = torch.Generator(device=dev).manual_seed(7)
    rows = {}
    for side in SIDES:
        hw = side * side
        target = torch.randint(0, 3, (3, 2 * side, 2 * side), device=dev, generator=gen)        # the step's targets: twice the decoder output
        for dtype in (torch.float32, torch.bfloat16):
            x = (torch.randn(3, C, side, side, device=dev, generator=gen).clamp_(min=0) * 0.5).to(dtype).contiguous(memory_format=torch.channels_last)
            x.requires_grad_(True)
            one = torch.ones((), device=dev)
            forms = {"kernel": lambda: nnf.supcon(x, target, TEMPERATURE)}
            if side == 96:
                forms["torch ops, chunked"] = lambda: supcon_torch(x, target, TEMPERATURE)
            for name, fwd in forms.items():
                with torch.no_grad():
                    f_med, f_min = _time(fwd, reps)
                y = fwd()

                def bwd():
                    x.grad = None
                    y.backward(one, retain_graph=True)

                b_med, b_min = _time(bwd, reps)
                pairs = float(hw) * hw
                rows[f"{name} {side}x{side} C{C} {str(dtype)[6:]}"] = {
                    "forward_us": round(f_med, 1), "forward_us_min": round(f_min, 1), "backward_us": round(b_med, 1), "backward_us_min": round(b_min, 1),
                    "forward_TFLOPs": round(2 * pairs * C / f_med / 1e6, 2), "forward_Gexp_per_s": round(pairs / f_med / 1e3, 1),
                    "backward_TFLOPs": round(8 * pairs * C / b_med / 1e6, 2), "loss": float(y)}
    return {"note": "HIP events around the Python call, median of 5 after 2 warm-ups; backward = two launches (roles swapped), each recomputes z "
                    "(2 HW^2 C flop) and runs the second product (2 HW^2 C): 8 HW^2 C in all", "rows": rows}


ARMS = {"off": {}, "supcon": dict(sup_con_loss_weight=0.5)}


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    keys = [only] if only else ["off", "supcon"]
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
                out = trainers[key].step(l_in, l_tg, ul)
            torch.cuda.synchronize()
            ms[key].append((time.perf_counter() - t0) * 1e3 / steps)
    res = {k: {"ms_per_step_rounds": [round(v, 2) for v in vs], "median": round(statistics.median(vs), 2)} for k, vs in ms.items()}
    if "supcon" in trainers:
        res["supcon"]["sup_con_loss"] = float(out["sup_con_loss"]) if "sup_con_loss" in out else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--only", default="", choices=[""] + sorted(ARMS), help="time one step arm only")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_times(dev)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
        if not args.only:
            off, on = res["step"]["off"]["median"], res["step"]["supcon"]["median"]
            res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
