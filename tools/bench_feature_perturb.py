"""Feature-perturbation cost (profiles/feature_perturb.md): the draw, the forward (copy + perturbed copy) and the backward (fold) launch
at the five decoder-input shapes of the 32 x 512^2 step, float32 and bfloat16, channels_last, each next to the torch-op form of the same
definition on the device; and the cfg3 CPS step with feature_perturb = 0.5 next to the same step with None -- two trainers in ONE
process, timed in interleaved rounds.

    python tools/bench_feature_perturb.py [--rounds 5] [--steps 3] [--no-step] [--no-kernel] [--only off|perturb|"off, second trainer"] [--out FILE]
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

# "off, second trainer": the plain step once more, from the SECOND trainer built in the process -- in the runs recorded so far that
# trainer's step is about 20 ms slower than the others', whatever its options (profiles/photometric.md); it holds that place so that
# the option does not
STEPS = {"off": None, "off, second trainer": None, "perturb": 0.5}
LEVELS = ((64, 256), (256, 128), (512, 64), (1024, 32), (2048, 16))       # (channels, side) of the decoder's inputs at 512 x 512 (resnet50)


def _timed(fn, reps):
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


def _row(nbytes, us, us_min):
    return {"bytes": nbytes, "us_median": round(us, 2), "us_min": round(us_min, 2), "GB_per_s": round(nbytes / us / 1e3, 1)}


def kernel_bandwidth(dev, batch, reps=20):
    from vq_seg_amd import _hip, nnf
    sizes = [(batch, c) for c, _s in LEVELS]
    key = dict(p=0.5, seed=42, stream=0, step=0, device=dev)
    rows = {}

    def both(fn):
        """fn under the HIP path and under py_feature_perturb=0 (the torch-op form on the device)"""
        out = {}
        for name, flag in (("hip", None), ("torch_ops", 0)):
            if flag is not None:
                _hip.PY_OPTS["py_feature_perturb"] = flag
            try:
                out[name] = _timed(fn, reps)
            finally:
                _hip.PY_OPTS.pop("py_feature_perturb", None)
        return out

    total = sum(b * c for b, c in sizes)
    rows["draw"] = {k: _row(4 * total, *v) for k, v in both(lambda: nnf.channel_keep(sizes, **key)).items()}        # one write per element
    _flat, scales = nnf.channel_keep(sizes, **key)
    for (c, s), scale in zip(LEVELS, scales):
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn(batch, c, s, s, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
            g = torch.randn(2 * batch, c, s, s, device=dev).to(dtype).contiguous(memory_format=torch.channels_last)
            nbytes = 3 * x.numel() * x.element_size()             # forward 1 read + 2 writes, backward 2 reads + 1 write per element
            name = f"{c}@{s}x{s} {str(dtype).removeprefix('torch.')}"
            fwd = both(lambda: nnf._ChannelDropoutCat.apply(x, scale, nnf.py_opt("py_feature_perturb", 1) == 1))
            fold_hip = lambda: nnf._dropout_launch("vqseg_channel_dropout_fold_f", g, scale,
                                                   torch.empty_like(x), batch, c, s, s)
            bwd = {"hip": _timed(fold_hip, reps), "torch_ops": _timed(lambda: nnf._dropout_fold_torch(g, scale), reps)}
            rows[name] = {"forward": {k: _row(nbytes, *v) for k, v in fwd.items()}, "backward": {k: _row(nbytes, *v) for k, v in bwd.items()}}
            del x, g
    return rows


def step_times(dev, rounds, steps, only=""):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    trainers = {}
    for key, p in STEPS.items():
        if only and key != only:
            continue
        cfg = CPSConfig(model=bench.model_cfg("cfg3"), recipe=wl["recipe"], total_iters=rounds * steps + 8, amp_dtype=torch.bfloat16, feature_perturb=p)
        trainers[key] = CPSTrainer(cfg, dev)
        for i in range(2):                                      # warm-up (k-means init, weight images, allocator)
            (l_in, l_tg), ul = batches[i % 2]
            trainers[key].step(l_in, l_tg, ul)
        torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for r in range(rounds):
        for key in [k for k in (list(STEPS) if r % 2 == 0 else list(STEPS)[::-1]) if k in trainers]:
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
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--only", default="", choices=[""] + list(STEPS), help="time one of the two steps only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_bandwidth(dev, args.batch)}
    if not args.no_step:
        res["step"] = step_times(dev, args.rounds, args.steps, args.only)
    if not args.no_step and not args.only:
        off, on = res["step"]["off"]["median"], res["step"]["perturb"]["median"]
        res["step"]["cost_ms"], res["step"]["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
        second = res["step"]["off, second trainer"]["median"]
        res["step"]["cost_ms off, second trainer vs off"] = round(second - off, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
