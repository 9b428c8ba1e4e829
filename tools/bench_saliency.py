"""RBD saliency cost (profiles/saliency.md) at the batch of a cfg3 step, 32 x 3 x 512 x 512:

  * every launch of nnf.saliency_rbd on its own, in microseconds, at n_segments 250 (a 16 x 16 grid) and 1024 (32 x 32): the region
    graph, the weights, the geodesic (3 launches per 64-cluster pivot block), the two row passes, the solve, the paint;
  * the whole nnf.saliency_rbd call (SLIC included) and nnf.rbd_from_labels (SLIC excluded);
  * the torch-op form of the same call on the device (utils.saliency.saliency_rbd_torch on GPU tensors);
  * the cfg3 CPS step with salient_mask=0.1 next to the plain step -- two trainers in ONE process, timed in interleaved rounds.

Timed with device events around back-to-back calls of the Python wrappers: the times include the wrappers' host work where the device
waits for it and are not kernel-trace times.

    python tools/bench_saliency.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--no-torch] [--only off|salient] [--out FILE]
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

SEGMENTS = (250, 1024)
THRESHOLD = 0.1


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
    return {"us": round(statistics.median(times), 1), "us_min": round(min(times), 1)}


def kernel_times(dev, batch, size, segments, reps=10, torch_form=True):
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import SyntheticCropWeed
    from vq_seg_amd.utils.saliency import saliency_rbd_torch
    images = SyntheticCropWeed(size, batch, dev, seed=42).unlabelled().float().contiguous(memory_format=torch.channels_last)
    out = {}
    with torch.no_grad():
        for k in segments:
            _sal, p = nnf.saliency_rbd(images, k, return_parts=True)
            gy, gx = p["grid"]
            lab, labels, stats, adj, g = p["lab"], p["labels"], p["stats"], p["adj"], p["geodesic"]
            wgt = nnf._rbd_weights(stats, adj)
            rows = {"grid": [gy, gx], "active_clusters_min": int((stats[..., 5] > 0).sum(1).min())}
            rows["region_graph"] = _time(lambda: nnf._rbd_region_graph(lab, labels, gy, gx), reps)
            rows["weights"] = _time(lambda: nnf._rbd_weights(stats, adj), reps)
            rows["geodesic (copy + %d launches)" % (3 * ((gy * gx + 63) // 64))] = _time(lambda: nnf._rbd_geodesic(wgt), reps)
            rows["background"] = _time(lambda: nnf._rbd_background(g, stats), reps)
            rows["contrast"] = _time(lambda: nnf._rbd_contrast(g, stats, p["w_bg"], size, size), reps)
            rows["solve"] = _time(lambda: nnf._rbd_solve(g, stats, adj, p["w_bg"], p["wctr"]), reps)
            rows["paint"] = _time(lambda: nnf._rbd_paint(p["xnorm"], labels, gy, gx), reps)
            rows["rbd_from_labels"] = _time(lambda: nnf.rbd_from_labels(lab, labels, (gy, gx)), reps)
            rows["slic alone"] = _time(lambda: nnf.slic(images, k), reps)
            rows["saliency_rbd (slic + rbd)"] = _time(lambda: nnf.saliency_rbd(images, k), reps)
            if torch_form:
                rows["torch-op form on the device"] = _time(lambda: saliency_rbd_torch(images, k), 2)
            out[f"n_segments={k}"] = rows
    return {"shape": [batch, 3, size, size], "note": "events around the Python wrappers", "rows": out}


ARMS = {"off": {}, "salient": dict(salient_mask=THRESHOLD, salient_segments=250)}


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    keys = [only] if only else ["off", "salient"]
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
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-op form (K broadcast minimum steps: slow at 1024)")
    ap.add_argument("--only", default="", choices=[""] + sorted(ARMS), help="time one step arm only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_saliency: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_times(dev, args.batch, args.size, SEGMENTS, torch_form=not args.no_torch)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
        if not args.only:
            off, on = res["step"]["off"]["median"], res["step"]["salient"]["median"]
            res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
