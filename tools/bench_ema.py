"""Cost of the averaged ("teacher") networks (profiles/ema_teacher.md): the Adam launch alone with and without averaging, and the cfg3
CPS step with ema_decay = None, with ema_decay = 0.999, with teacher_pseudo_labels = True, and -- the alternative the in-launch
average replaces -- the same teacher kept by torch._foreach_lerp_ after the step with its weight images repacked lazily.  All arms
live in ONE process and are timed in interleaved rounds.

    python tools/bench_ema.py [--rounds 5] [--steps 3] [--no-step] [--no-launch] [--only off|ema|pseudo|lerp] [--out FILE]
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

DECAY = 0.999
ARMS = ("off", "ema", "pseudo", "lerp")


def _trainer(dev, arm, iters):
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    wl = bench.WORKLOADS["cfg3"]
    kw = {"off": {}, "ema": dict(ema_decay=DECAY), "pseudo": dict(ema_decay=DECAY, teacher_pseudo_labels=True),
          "lerp": dict(ema_decay=DECAY, teacher_pseudo_labels=True)}[arm]
    tr = CPSTrainer(CPSConfig(model=bench.model_cfg("cfg3"), recipe=wl["recipe"], total_iters=iters, amp_dtype=torch.bfloat16, **kw), dev)
    if arm == "lerp":                                          # the teacher exists and gives the pseudo labels, but the launch does not keep it
        for o in tr.opts:
            o.attach_average(None)
    return tr


def _lerp_teachers(tr):
    """what the in-launch average replaces: one foreach pass over the fp32 masters after the step, every teacher image dropped"""
    from vq_seg_amd import _wcache
    with torch.no_grad():
        for avg in tr.averages:
            torch._foreach_lerp_([p.teacher for p in avg.pairs], [p.student.detach() for p in avg.pairs], 1.0 - DECAY)
            _wcache.invalidate(avg.module)
            avg.updates += 1


def _step(tr, arm, batch):
    (l_in, l_tg), ul = batch
    tr.step(l_in, l_tg, ul)
    if arm == "lerp":
        _lerp_teachers(tr)


def _table_bytes(opt):
    """bytes the launch of `opt` moves, counted from its tables: 28 B of fp32 state per stepped element + the student's images, and with
    an average 8 B per averaged element (4 B for a copy record: e is not read; + 4 B for the p an average-only record reads) + its images"""
    images = ema = t_images = 0
    for tab in opt._tables.values():
        for imgs in tab["images"]:
            images += sum(b.numel() * 2 for b in (imgs or {}).values())
        for t, imgs in tab.get("teachers", ()):
            t_images += sum(b.numel() * 2 for b in (imgs or {}).values())
    stepped = {id(p) for g in opt.param_groups for p in g["params"] if p.grad is not None}
    state = 28 * sum(p.numel() for g in opt.param_groups for p in g["params"] if p.grad is not None)
    if opt._average is not None:
        for pr in opt._average.pairs:
            ema += pr.student.numel() * ((4 if pr.copy else 8) + (0 if id(pr.student) in stepped else 4))
    return dict(state=state, images=images, ema=ema, teacher_images=t_images)


def launch_times(dev, trainers, reps=20):
    """the Adam launch of network 1 alone, on the state the warm-up steps left (the gradients stay in the buckets): plain, with the
    average, with the average and the teacher's images (the teacher has run forwards, so its image kinds are known).  HIP events around
    `opt.step()`: where the call's host time exceeds the kernel's (profiles/ema_teacher.md) the figure is the host's, and the kernel alone is
    read from a kernel trace of `--only <arm>`"""
    rows = {}
    for name, arm, attach in (("adam", "ema", False), ("adam + average", "ema", True), ("adam + average + teacher images", "pseudo", True)):
        tr = trainers.get(arm)
        if tr is None:
            continue
        opt, avg = tr.opts[0], tr.averages[0]
        opt.attach_average(avg if attach else None)
        for _ in range(3):
            opt.step()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        b = _table_bytes(opt)
        total = sum(b.values())
        us = statistics.median(times)
        rows[name] = {"bytes": b, "bytes_total": total, "elements": b["state"] // 28, "us_median": round(us, 1), "us_min": round(min(times), 1),
                      "GB_per_s": round(total / us / 1e3, 1), "bytes_per_element": round(total / (b["state"] / 28), 2)}
        opt.attach_average(avg)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-launch", action="store_true")
    ap.add_argument("--only", default="", choices=("",) + ARMS, help="time one arm of the step only (for a kernel trace of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench
    from vq_seg_amd.trainer import SyntheticCropWeed
    dev = torch.device("cuda:0")
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    arms = [a for a in ARMS if not args.only or a == args.only]
    if args.no_step and not args.only:
        arms = ["ema", "pseudo"]
    trainers = {}
    for arm in arms:
        trainers[arm] = _trainer(dev, arm, args.rounds * args.steps + 64)
        for i in range(2):                                      # warm-up (k-means init, weight images, the teacher's first copy, allocator)
            _step(trainers[arm], arm, batches[i % 2])
        torch.cuda.synchronize()
    res = {"decay": DECAY}
    if not args.no_step:
        ms = {a: [] for a in arms}
        for r in range(args.rounds):
            for arm in (arms if r % 2 == 0 else arms[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    _step(trainers[arm], arm, batches[i % 2])
                torch.cuda.synchronize()
                ms[arm].append((time.perf_counter() - t0) * 1e3 / args.steps)
        res["step"] = {a: {"ms_per_step_rounds": [round(v, 2) for v in vs], "median": round(statistics.median(vs), 2)} for a, vs in ms.items()}
        if "off" in ms:
            off = res["step"]["off"]["median"]
            for a in arms:
                if a != "off":
                    res["step"][a]["cost_ms"] = round(res["step"][a]["median"] - off, 2)
    if not args.no_launch:                                      # last: it steps the optimisers on stale gradients
        res["launch"] = launch_times(dev, trainers)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
