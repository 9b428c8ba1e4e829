"""Boundary-metric cost (profiles/boundary.md) at 32 x 512 x 512 and 4 x 966 x 1296 uint8 class maps with C = 3:

  * every launch on its own -- boundaries, the row pass, the column pass, the counts -- and the whole utils.boundary.boundary_stats
    call, in microseconds and GB/s of algorithmic bytes, on label maps (synthetic blob maps with the prediction = the target shifted
    by 3 pixels; a random 3-class map; one value everywhere, where every plane is empty) and, for the two passes of the distance
    transform, on the seed planes that are the pruned column search's worst cases (a single seed in one corner; seeds in the first
    and the last row only);
  * the same boundary_stats table as torch device ops (utils.boundary's torch-op form on GPU tensors; checked equal here);
  * scipy.ndimage.distance_transform_edt on the host for the same 2 C planes per image, the device-to-host copy of the seed planes
    and the copy back of the distances included;
  * evaluate.test_loop(fused=True) on the cfg3 network with and without boundary=True.

Algorithmic bytes per pixel of a uint8 map with C classes, from the shapes: boundaries 1 + C; row pass (1 + 2) C (the row flags are
small); column pass (2 + 4) C (the tile's rows of g are re-read from cache); counts 1 + 1 + 2 x (1 + 1 + 4 + 4) = 22 (a pixel touches the
planes of its predicted and of its target class only); boundary_stats = 2 x (boundaries + rows + columns) + counts = 2 + 20 C + 22.

Timed with device events around back-to-back calls of the Python wrappers: the times include the wrappers' host work where the device
waits for it and are not kernel-trace times.

    python tools/bench_boundary.py [--reps 20] [--shape I] [--map KIND] [--no-torch-form] [--no-scipy] [--no-loop] [--out FILE]
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

C = 3
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


def blob_pair(dev, b, h, w):
    from tools.bench_regions import blob_map
    target = blob_map(dev, b, h, w)
    return torch.roll(target, (3, 3), dims=(1, 2)).contiguous(), target


def random_pair(dev, b, h, w):
    g = torch.Generator(device="cpu").manual_seed(41)
    return tuple(torch.randint(0, C, (b, h, w), generator=g, dtype=torch.uint8).to(dev) for _ in range(2))


def constant_pair(dev, b, h, w):
    one = torch.ones((b, h, w), dtype=torch.uint8, device=dev)
    return one, one.clone()


def corner_seed(dev, planes, h, w):
    s = torch.zeros((planes, h, w), dtype=torch.uint8, device=dev)
    s[:, 0, 0] = 1
    return s


def first_last_rows(dev, planes, h, w):
    s = torch.zeros((planes, h, w), dtype=torch.uint8, device=dev)
    s[:, 0, ::2] = 1
    s[:, -1, 1::3] = 1
    return s


def _passes(seeds, reps):
    """the row launch and the column launch on (planes, h, w) seeds, through the library itself on buffers made once"""
    from vq_seg_amd import _hip
    planes, h, w = seeds.shape
    px = planes * h * w
    g = torch.empty((planes, h, w), dtype=torch.int16, device=seeds.device)
    has = torch.empty((planes, h), dtype=torch.uint8, device=seeds.device)
    d2 = torch.empty((planes, h, w), dtype=torch.int32, device=seeds.device)
    dev = seeds.device
    rows = lambda: _hip.launch("vqseg_boundary_edt_rows_u8", dev, seeds.data_ptr(), planes, h, w, g.data_ptr(), has.data_ptr())
    cols = lambda: _hip.launch("vqseg_boundary_edt_cols_i32", dev, g.data_ptr(), has.data_ptr(), planes, h, w, d2.data_ptr())
    out = {"row pass": _row(*_time(rows, reps), px * 3)}
    out["column pass"] = _row(*_time(cols, reps), px * 6)
    out["rows with a seed"] = round(float(has.float().mean()), 4)
    return out


def kernel_rates(dev, reps, only_map, only_shape, torch_form, scipy_host):
    from vq_seg_amd import nnf
    from vq_seg_amd.utils import boundary
    out = {}
    for b, h, w in (SHAPES if only_shape < 0 else SHAPES[only_shape:only_shape + 1]):
        px = b * h * w
        for kind, make in (("blobs, shifted by 3", blob_pair), ("random", random_pair), ("one value", constant_pair)):
            if only_map and only_map not in kind:
                continue
            p, t = make(dev, b, h, w)
            rows = {}
            bp, bg = nnf.class_boundaries(p, C, (255,)), nnf.class_boundaries(t, C, (255,))
            dp, dg = nnf.edt_sq(bp), nnf.edt_sq(bg)
            rows["boundary pixels per image"] = round(float(bg.sum()) / b, 1)
            rows["boundaries"] = _row(*_time(lambda: nnf.class_boundaries(t, C, (255,)), reps), px * (1 + C))
            rows.update(_passes(bg.view(b * C, h, w), reps))
            n = px
            counts = lambda: nnf._launch("vqseg_boundary_counts_i32", dev, p.data_ptr(), 1, t.data_ptr(), 1, bp.data_ptr(), bg.data_ptr(), dp.data_ptr(),
                                         dg.data_ptr(), b, h, w, C, 4, 4, 1, 255, 0, 0, 0, table.data_ptr())
            table = torch.empty((b, C, 8), dtype=torch.int32, device=dev)
            rows["counts"] = _row(*_time(counts, reps), n * 22)
            whole = px * (2 + 20 * C + 22)
            rows["boundary_stats"] = _row(*_time(lambda: boundary.boundary_stats(p, t, C, 2.0), reps), whole)
            want = nnf.boundary_counts(p, t, C, 4, 4, (255,))
            assert torch.equal(table, want), "the counts launch on its own differs from boundary_counts"
            if torch_form:
                assert torch.equal(boundary.counts_torch(p, t, C, 4, 4, (255,)), want), "torch-op table differs from the kernels'"
                rows["torch ops: the same table"] = _row(*_time(lambda: boundary.counts_torch(p, t, C, 4, 4, (255,)), 2), whole)
            if scipy_host:
                from scipy import ndimage

                def host():
                    for seeds in (bp, bg):
                        s = seeds.cpu().numpy()
                        d = torch.empty(s.shape, dtype=torch.float64)
                        for idx in ((i, c) for i in range(b) for c in range(C)):
                            if s[idx].any():
                                d[idx] = torch.from_numpy(ndimage.distance_transform_edt(s[idx] == 0))
                        d.to(dev)
                    torch.cuda.synchronize()
                t0 = time.perf_counter()
                host()
                rows["scipy on the host: 2 C transforms per image, copies included"] = {"us": round((time.perf_counter() - t0) * 1e6, 1), "runs": 1}
            out[f"{b} x {h} x {w}, {kind}"] = rows
            print(f"bench_boundary: {b} x {h} x {w}, {kind} done", file=sys.stderr, flush=True)
            del p, t, bp, bg, dp, dg, table, want
            torch.cuda.empty_cache()
        for kind, make in (("a single seed in one corner", corner_seed), ("seeds in the first and last row only", first_last_rows)):
            if only_map and only_map not in kind:
                continue
            out[f"{b * C} planes of {h} x {w}, {kind}"] = _passes(make(dev, b * C, h, w), reps)
            torch.cuda.empty_cache()
    return {"classes": C, "tolerance": 2.0, "note": "events around the Python wrappers (the two passes and the counts: around the launch path on "
            "buffers made once); GB/s are the algorithmic bytes over the time", "rows": out}


def loop_times(dev, reps):
    """evaluate.test_loop(fused=True) on the cfg3 network over two synthetic batches, with and without boundary=True"""
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [data.labelled() for _ in range(2)]
    tr = CPSTrainer(CPSConfig(model=bench.model_cfg("cfg3"), recipe="v1", total_iters=16, amp_dtype=torch.bfloat16), dev)
    rows = {}
    for key, kw in (("fused", {}), ("fused, boundary=True", dict(boundary=True))):
        times = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tr.evaluate(batches, fused=True, **kw)
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        rows[key] = {"ms": round(statistics.median(times), 2), "ms_min": round(min(times), 2), "result": {k: v for k, v in res.items() if "boundary" in k or
                                                                                                        k in ("test_miou", "test_hausdorff")}}
    return {"shape": list(batches[0][0].shape), "batches": len(batches), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", type=int, default=-1, help="only this entry of SHAPES")
    ap.add_argument("--map", default="", help="only the inputs whose name contains this")
    ap.add_argument("--no-torch-form", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_boundary: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_rates(dev, args.reps, args.map, args.shape, not args.no_torch_form, not args.no_scipy)}
    if not args.no_loop:
        res["test_loop"] = loop_times(dev, 5)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
