"""Connected-region cost (profiles/regions.md) at 32 x 512 x 512 and 4 x 966 x 1296 uint8 class maps, on three kinds of map: synthetic
blob maps (data/synthetic.py's labels), a random 3-class map at density 0.59, which leaves one giant 4-connected region per image
and is the hard case for the merge across tile borders, and one value everywhere, where every link lands in one tree:

  * every entry point on its own -- roots (local + merge + flatten), ids (flags + scan + rank + gather), areas, table (capacity 1024)
    and the filter gather -- and the whole utils.regions.label_regions / remove_small_regions call, in microseconds and GB/s of
    algorithmic bytes; the split of an entry point into its launches comes from a kernel trace of one map kind
    (rocprofv3 --kernel-trace --stats -- python tools/bench_regions.py --no-step --no-torch-form --shape 0 --map blobs);
  * the same two calls as torch device ops (utils.regions' torch-op form on GPU tensors: neighbourhood minima with pointer jumping);
  * Predictor on the cfg3 network with and without min_area=64;
  * the cfg3 CPS step with pseudo_min_area=64 next to the plain step -- every arm in child processes of its own, the arms alternating
    (see step_times for why not two trainers in one process) -- and the entry-point calls of one step of each arm, counted at
    nnf._launch / _hip.launch.

Algorithmic bytes per pixel of a uint8 map, from the shapes: roots 1 + 4 (local) + 4 + 4 (flatten) = 13 (the merge touches the tile
borders only); ids 4 (flags) + 4 (rank) + 4 + 4 (gather) = 16; areas 4 (memset) + 4 = 8; table 2 x (4 + 4) = 16 (the rows are small);
filter 1 + 4 + 4 + 1 = 10; label_regions = roots + ids = 29; remove_small_regions = roots + areas + filter = 31.

Timed with device events around back-to-back calls of the Python wrappers: the times include the wrappers' host work where the device
waits for it and are not kernel-trace times.

    python tools/bench_regions.py [--rounds 3] [--steps 6] [--no-step] [--no-kernel] [--no-predict] [--map KIND] [--shape I] [--no-torch-form] [--out FILE]
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_AREA, CAPACITY = 64, 1024
SHAPES = [(32, 512, 512), (4, 966, 1296)]


def _time(fn, reps):
    for _ in range(2):
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


def blob_map(dev, b, h, w):
    """data/synthetic.py's labels, tiled / cropped to h x w"""
    from vq_seg_amd.trainer import SyntheticCropWeed
    side = 512
    tgt = SyntheticCropWeed(side, b, dev, seed=42).labelled()[1].to(torch.uint8)
    reps = (1, (h + side - 1) // side, (w + side - 1) // side)
    return tgt.repeat(*reps)[:, :h, :w].contiguous()


def random_map(dev, b, h, w, density=0.59):
    g = torch.Generator(device="cpu").manual_seed(59)
    u = torch.rand((b, h, w), generator=g)
    return torch.where(u < density, 1, torch.where(u < density + (1 - density) / 2, 0, 2)).to(torch.uint8).to(dev)


def constant_map(dev, b, h, w):
    return torch.ones((b, h, w), dtype=torch.uint8, device=dev)


def kernel_rates(dev, reps=20, only_map="", only_shape=-1, torch_form=True):
    from vq_seg_amd import nnf
    from vq_seg_amd.utils import regions
    out = {}
    for b, h, w in (SHAPES if only_shape < 0 else SHAPES[only_shape:only_shape + 1]):
        px = b * h * w
        for kind, make in (("blobs", blob_map), ("random 0.59", random_map), ("one value", constant_map)):
            if only_map and only_map not in kind:
                continue
            v = make(dev, b, h, w)
            rows = {}
            for conn in (4, 8):
                roots = nnf.region_roots(v, conn)
                ids, counts = nnf.region_ids(roots)
                areas = nnf.region_areas(roots)
                rows[f"regions per image, {conn}-connected"] = [int(counts.min()), int(counts.max())]
                rows[f"roots, {conn}"] = _row(*_time(lambda: nnf.region_roots(v, conn), reps), px * 13)
                if conn == 4:
                    rows["ids"] = _row(*_time(lambda: nnf.region_ids(roots), reps), px * 16)
                    rows["areas"] = _row(*_time(lambda: nnf.region_areas(roots), reps), px * 8)
                    rows[f"table, capacity {CAPACITY}"] = _row(*_time(lambda: nnf.region_table(v, roots, ids, counts, CAPACITY), reps), px * 16)
                    rows["filter"] = _row(*_time(lambda: nnf.filter_regions_from(v, roots, areas, MIN_AREA, "neighbour"), reps), px * 10)
                rows[f"label_regions, {conn}"] = _row(*_time(lambda: regions.label_regions(v, conn), reps), px * 29)
                rows[f"remove_small_regions, {conn}"] = _row(*_time(lambda: regions.remove_small_regions(v, MIN_AREA, conn), reps), px * 31)
            # the torch-op form on the device: the same numbers (checked here), its own time over the same bytes
            roots_t = None
            if torch_form:
                roots_t = regions.roots_torch(v, 4)
                assert torch.equal(roots_t, nnf.region_roots(v, 4)), "torch-op roots differ from the kernels'"
                rows["torch ops: roots + ids, 4"] = _row(*_time(lambda: regions.ids_torch(regions.roots_torch(v, 4)), 2), px * 29)
            out[f"{b} x {h} x {w}, {kind}"] = rows
            print(f"bench_regions: {b} x {h} x {w}, {kind} done", file=sys.stderr, flush=True)
            del v, roots, ids, areas, roots_t
            torch.cuda.empty_cache()
    return {"min_area": MIN_AREA, "note": "events around the Python wrappers; GB/s are the algorithmic bytes over the time, so the torch-op "
            "rows show the same bytes over their longer time", "rows": out}


def _counting(names):
    """count entry-point calls at the one launch path while the block runs"""
    import contextlib
    from vq_seg_amd import _hip, nnf

    @contextlib.contextmanager
    def ctx():
        real = _hip.launch

        def counted(name, *a, **k):
            names[name] += 1
            return real(name, *a, **k)
        _hip.launch, nnf._launch = counted, counted
        try:
            yield
        finally:
            _hip.launch, nnf._launch = real, real
    return ctx()


ARMS = {"off": {}, "pseudo_min_area": dict(pseudo_min_area=MIN_AREA)}


def step_child(dev, arm, steps, predict):
    """one arm in this process: a trainer, two warm-up steps, the entry-point calls of one step, `steps` timed steps (and Predictor)"""
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [(data.labelled(), data.unlabelled()) for _ in range(2)]
    tr = CPSTrainer(CPSConfig(model=bench.model_cfg("cfg3"), recipe="v1", total_iters=steps + 16, amp_dtype=torch.bfloat16, **ARMS[arm]), dev)
    for i in range(2):                                          # warm-up (k-means init, weight images, allocator)
        (l_in, l_tg), ul = batches[i % 2]
        tr.step(l_in, l_tg, ul)
    torch.cuda.synchronize()
    names = collections.Counter()
    with _counting(names):
        (l_in, l_tg), ul = batches[0]
        tr.step(l_in, l_tg, ul)
    torch.cuda.synchronize()
    ms = []
    for i in range(steps):
        (l_in, l_tg), ul = batches[i % 2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    res = {"ms_per_step": [round(v, 2) for v in ms], "entry_point_calls": sum(names.values()),
           "region_calls": {k: v for k, v in sorted(names.items()) if k.startswith("vqseg_region_") and k != "vqseg_region_graph_f"}}
    if predict:
        images, rows = batches[0][1], {}
        for key, kw in (("plain", {}), (f"min_area={MIN_AREA}", dict(min_area=MIN_AREA, min_area_fill="neighbour"))):
            med, mn = _time(lambda: tr.predict(images, **kw), 10)
            rows[key] = {"us": round(med, 1), "us_min": round(mn, 1)}
        res["predict"] = {"shape": list(images.shape), "rows": rows}
    return res


def step_times(rounds, steps, predict=True):
    """Each arm in a child process of its own, the arms alternating, `rounds` children per arm.  Two trainers in ONE process do not
    measure this option: the trainer that is built second runs about 20 ms per step slower than the first whatever its options are
    (measured: the arm with the option on and min_area 1, built third, ran at the plain step's time), which a first version of this
    tool reported as the option's cost."""
    import subprocess
    runs = {k: [] for k in ARMS}
    keys = list(ARMS)
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", key, "--steps", str(steps)] + ([] if predict and r == 0 and key == "off" else ["--no-predict"])
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            runs[key].append(json.loads(out.strip().splitlines()[-1]))
            print(f"bench_regions: step arm {key}, round {r} done", file=sys.stderr, flush=True)
    res = {}
    for key, rs in runs.items():
        med = [statistics.median(x["ms_per_step"]) for x in rs]
        res[key] = {"entry_point_calls": rs[0]["entry_point_calls"], "region_calls": rs[0]["region_calls"],
                    "ms_per_step_by_process": [x["ms_per_step"] for x in rs], "median": round(statistics.median(med), 2)}
    off, on = res["off"]["median"], res["pseudo_min_area"]["median"]
    res["cost_ms"], res["cost_percent"] = round(on - off, 2), round(100 * (on - off) / off, 2)
    if predict:
        res["predict"] = runs["off"][0]["predict"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--map", default="", help="only the map kinds whose name contains this (blobs, random, one value): for a kernel trace of one kind")
    ap.add_argument("--shape", type=int, default=-1, help="only this entry of SHAPES")
    ap.add_argument("--no-torch-form", action="store_true", help="leave the torch-op rows out (a kernel trace of them is thousands of launches)")
    ap.add_argument("--child", default="", choices=[""] + sorted(ARMS), help="(used by the tool itself) time one step arm in this process")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    if args.child:
        print(json.dumps(step_child(dev, args.child, args.steps, not args.no_predict)))
        return
    res = {} if args.no_kernel else {"kernel": kernel_rates(dev, only_map=args.map, only_shape=args.shape, torch_form=not args.no_torch_form)}
    if not args.no_step:
        res["step"] = step_times(args.rounds, args.steps, predict=not args.no_predict)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
