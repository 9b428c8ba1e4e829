"""SLIC / superpixel-mean cost (profiles/superpixel.md) at the batch of a cfg3 step, 32 x 3 x 512 x 512, K = 1600 (a 40 x 40 grid),
compactness 10, 10 iterations:

  * the Lab, assign and update launches on their own and the whole nnf.slic call (1 + 10 x 2 + 1 launches), in microseconds and GB/s
    of algorithmic bytes;
  * nnf.segment_mean forward (sums + broadcast) and backward (the same two launches on the gradient) on 32 x 3 x 512 x 512 logits,
    NCHW and channels_last, next to the same pooling as torch device ops (index_add_: utils.superpixel's torch-op form on GPU tensors);
  * the cfg3 CPS step with superpixel_mean=1600 next to the plain step -- two trainers in ONE process, timed in interleaved rounds.

Algorithmic bytes, from the shapes: Lab reads and writes 3 floats per pixel (24 B); assign reads 3 floats and writes one int32
(16 B; the centres are 32 KB per image and stay in cache); update reads, per cluster, the labels of its 3 x 3 cells and the Lab values of
its own pixels: 9 x 4 + 12 B per pixel of the image (48 B); the segment sums read C floats and a label per pixel, the broadcast reads
the label and writes C floats (the tables are small): (8 C + 8) B per pixel for the pair, forward or backward.

Timed with device events around back-to-back calls of the Python wrappers: the times include the wrappers' host work where the device
waits for it and are not kernel-trace times.

    python tools/bench_superpixel.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--only off|superpixel] [--out FILE]
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

K, COMPACTNESS, ITERS = 1600, 10.0, 10


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


def _row(med, mn, nbytes):
    return {"us": round(med, 1), "us_min": round(mn, 1), "bytes": nbytes, "GB_per_s": round(nbytes / med / 1e3, 1)}


def kernel_rates(dev, batch, size, reps=20):
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import SyntheticCropWeed
    from vq_seg_amd.utils.superpixel import _SegmentMeanTorch
    images = SyntheticCropWeed(size, batch, dev, seed=42).unlabelled().float().contiguous(memory_format=torch.channels_last)
    px = batch * size * size
    gy, gx, weight, _ = nnf.slic_settings(size, size, K, COMPACTNESS, ITERS)
    lab, centers = nnf._slic_lab(images, gy, gx)
    labels = nnf._slic_assign(lab, centers, gy, gx, weight)
    rows = {"grid": [gy, gx]}
    with torch.no_grad():
        rows["lab (channels_last images)"] = _row(*_time(lambda: nnf._slic_lab(images, gy, gx), reps), px * 24)
        rows["assign"] = _row(*_time(lambda: nnf._slic_assign(lab, centers, gy, gx, weight, labels), reps), px * 16)
        scratch = centers.clone()
        rows["update"] = _row(*_time(lambda: nnf._slic_update(lab, labels, scratch, gy, gx), reps), px * 48)
        rows[f"slic, {ITERS} iterations"] = _row(*_time(lambda: nnf.slic(images, K, COMPACTNESS, ITERS), reps),
                                                 px * (24 + (ITERS + 1) * 16 + ITERS * 48))
    labels = nnf.slic(images, K, COMPACTNESS, ITERS)[0]
    c, k_eff = 3, gy * gx
    one = None
    for layout in ("nchw", "channels_last"):
        x = torch.randn(batch, c, size, size, device=dev) * 3
        if layout == "channels_last":
            x = x.contiguous(memory_format=torch.channels_last)
        x.requires_grad_(True)
        one = torch.randn_like(x)
        for name, fwd in (("segment_mean", lambda: nnf.segment_mean(x, labels, k_eff)),
                          ("torch ops (index_add_)", lambda: _SegmentMeanTorch.apply(x, labels, k_eff))):
            with torch.no_grad():
                f_med, f_min = _time(fwd, reps)
            y = fwd()

            def bwd():
                x.grad = None
                y.backward(one, retain_graph=True)

            b_med, b_min = _time(bwd, reps)
            nbytes = px * (8 * c + 8)
            rows[f"{name}, {layout}"] = {"forward": _row(f_med, f_min, nbytes), "backward": _row(b_med, b_min, nbytes)}
            del y
    return {"shape": [batch, 3, size, size], "num_components": K, "note": "events around the Python wrappers; GB/s are the algorithmic "
            "bytes of the fused form over the time, so the torch-op rows show the same bytes over their longer time", "rows": rows}


ARMS = {"off": {}, "superpixel": dict(superpixel_mean=K, superpixel_compactness=COMPACTNESS, superpixel_iters=ITERS)}


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    keys = [only] if only else ["off", "superpixel"]
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
    if not torch.cuda.is_available():
        raise SystemExit("bench_superpixel: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_rates(dev, args.batch, args.size)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
        if not args.only:
            off, on = res["step"]["off"]["median"], res["step"]["superpixel"]["median"]
            res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
