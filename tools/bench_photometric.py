"""Photometric strong augmentation cost (profiles/photometric.md), all at 32 x 3 x 512 x 512: the kernel call with all ops on, colour
only and blur only, in both layouts, in us and GB/s of algorithmic bytes (one read and one write per element, one extra read when a
contrast is on: the mean pass); the mean pass and the main pass apart; the same transform as torch device ops; and the cfg3 CPS step
with hard_aug = "photometric" next to the plain step (and both with cutmix_ratio = 0.25) -- all trainers in ONE process, timed in
interleaved rounds.

The two passes apart: a call whose rows have c = 1 launches the main pass alone, so "main pass" is the call timed with the same rows
but c = 1 (the contrast op itself is three multiply-adds per pixel of a pass bound elsewhere), and "mean pass" the difference to the whole
call; the exact per-kernel durations come from a kernel trace of `--no-step --no-torch` (photometric_mean_kernel / photometric_kernel).

    python tools/bench_photometric.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--no-torch] [--only KEY] [--out FILE]
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

# "off, second trainer": the plain step once more, from the SECOND trainer built in the process -- in every run recorded so far the
# second trainer's step is about 20 ms slower than the others', whatever its options (profiles/photometric.md); it holds that place so
# that no option does
STEPS = {"off": dict(), "off, second trainer": dict(), "photometric": dict(hard_aug="photometric"), "cutmix": dict(cutmix_ratio=0.25),
         "photometric+cutmix": dict(hard_aug="photometric", cutmix_ratio=0.25)}
ALL = (1.3, 0.7, 1.4, 0.2, 0.0, 1.5)                          # every colour op and a blur of R = 5
ROWS = {"all ops (R = 5)": ALL, "all ops, sigma 2.0 (R = 6)": ALL[:5] + (2.0,), "colour only": ALL[:5] + (0.0,),
        "blur only (R = 5)": (1.0, 1.0, 1.0, 0.0, 0.0, 1.5), "identity (copy)": (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)}


def _timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times)


def kernel_times(dev, batch, size, reps=20):
    """HIP-event time per call of _hip.photometric (its launches back to back on one stream)"""
    from vq_seg_amd import _hip
    from vq_seg_amd.data import augmentations as A
    img = torch.rand(batch, 3, size, size, device=dev)
    tensors = {"nchw": img, "channels_last": img.contiguous(memory_format=torch.channels_last)}
    cases = {name: [row] * batch for name, row in ROWS.items()}
    cases["the step's per-sample draws"] = A.step_photometric(batch, 42, 0, 0, "sample")
    rows_out = {}
    for lname, t in tensors.items():
        out = torch.empty_like(t)
        for name, rows in cases.items():
            contrast = any(r[1] != 1.0 for r in rows)
            ms, ms_min = _timed(lambda: _hip.photometric(t, rows, out=out), reps)
            nbytes = (3 if contrast else 2) * t.numel() * 4
            row = {"bytes": nbytes, "us_median": round(ms * 1e3, 1), "us_min": round(ms_min * 1e3, 1), "GB_per_s": round(nbytes / ms / 1e6, 1)}
            if contrast:                                        # the same rows with c = 1: the main pass alone
                main = [(r[0], 1.0) + tuple(r[2:]) for r in rows]
                ms1, ms1_min = _timed(lambda: _hip.photometric(t, main, out=out), reps)
                b1 = 2 * t.numel() * 4
                row["main_pass"] = {"bytes": b1, "us_median": round(ms1 * 1e3, 1), "us_min": round(ms1_min * 1e3, 1), "GB_per_s": round(b1 / ms1 / 1e6, 1)}
                d = max(ms - ms1, 1e-6)
                row["mean_pass_by_difference"] = {"bytes": t.numel() * 4, "us_median": round(d * 1e3, 1), "GB_per_s": round(t.numel() * 4 / d / 1e6, 1)}
            rows_out[f"{name}, {lname}"] = row
    return rows_out


def torch_times(dev, batch, size, reps=5):
    """the same transform with torch device ops (the CPU form of data.augmentations run on the device, sample by sample as it is
    written): what the kernel replaces -- about a dozen elementwise launches and two stencils per sample"""
    from vq_seg_amd import _hip
    from vq_seg_amd.data import augmentations as A
    t = torch.rand(batch, 3, size, size, device=dev).contiguous(memory_format=torch.channels_last)
    res = {}
    for name in ("all ops (R = 5)", "colour only", "blur only (R = 5)"):
        rows, radii, taps = _hip.photometric_rows([ROWS[name]] * batch, batch, size, size)
        ms, ms_min = _timed(lambda: A._photometric_torch(t, rows, radii, taps), reps, warm=1)
        res[f"{name}, channels_last"] = {"us_median": round(ms * 1e3, 1), "us_min": round(ms_min * 1e3, 1)}
    return res


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
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--only", default="", choices=[""] + list(STEPS), help="time one of the steps only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {}
    if not args.no_kernel:
        res["kernel"] = kernel_times(dev, args.batch, args.size)
    if not args.no_torch:
        res["torch_device_ops"] = torch_times(dev, args.batch, args.size)
    if not args.no_step:
        res["step"] = st = step_times(dev, args.rounds, args.steps, args.only)
        if not args.only:
            for on, off in (("off, second trainer", "off"), ("photometric", "off"), ("photometric+cutmix", "cutmix")):
                d = st[on]["median"] - st[off]["median"]
                st[f"cost_ms {on} vs {off}"], st[f"cost_percent {on} vs {off}"] = round(d, 2), round(100 * d / st[off]["median"], 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
