"""Panoptic-quality cost (profiles/instances.md) at 32 x 512 x 512 and 4 x 966 x 1296 uint8 class maps with C = 3:

  * every entry point on its own -- the vote pass, the overlap pass (candidates + second pass), the match and the tally -- and the
    whole utils.instances.panoptic_stats call (regions of both sides included), in microseconds and GB/s of the bytes each must read,
    on tools/bench_boundary.py's maps: synthetic blob maps with the prediction = the target shifted by 3 pixels; two random 3-class
    maps (tens of thousands of regions per image: the capacity is raised to the matching's limit of 65535 and the images that still
    overflow are reported); one value everywhere (one giant region on both sides);
  * nnf.region_areas on the prediction's roots at the same shape in the same session: the yardstick of the two image passes (one pass
    over one int32 map with the same run folding), with the ratio of the time per byte;
  * the same tables as torch device ops (utils.instances' torch-op form on GPU tensors; checked equal here);
  * the numpy / scipy form on the host: scipy.ndimage.label per image and class and a dense pair count, the copy of both maps included;
  * evaluate.test_loop(fused=True) on the cfg3 network with and without panoptic=True.

Bytes per pixel, from the shapes: vote 4 + 4 (both id maps; the target is read only where a prediction region lies on no ground-truth
region); overlap 4 + 4 (the candidate table is small and cached); region_areas 4; panoptic_stats = 2 x (the thing map 1 + 1, roots 13,
ids 16, table 16) + 1 (void) + 16 = 111.  Match and tally read b x capacity rows and have no pixel rate.

Timed with device events around back-to-back calls of the library's entry points on buffers made once (the whole calls: around the
Python call): the times include the host work where the device waits for it and are not kernel-trace times.

    python tools/bench_instances.py [--reps 20] [--shape I] [--map KIND] [--no-torch-form] [--no-host] [--no-loop] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_boundary import C, SHAPES, _row, _time, blob_pair, constant_pair, random_pair  # noqa: E402

CAPACITY = 1024
MAX_CAPACITY = 65535


def host_form(p, t, things=(1, 2), void=(255,)):
    """the numpy / scipy form: labels per image and class, a dense pair count over the regions that meet, all pairs tested"""
    from scipy import ndimage
    p, t = p.cpu().numpy(), t.cpu().numpy()
    tally = np.zeros((p.shape[0], C, 3), dtype=np.int64)
    for k in range(p.shape[0]):
        is_void = np.isin(t[k], void)
        for c in things:
            pl, n_p = ndimage.label(p[k] == c)
            gl, n_g = ndimage.label(t[k] == c)
            pa = np.bincount(pl.reshape(-1), minlength=n_p + 1)
            ga = np.bincount(gl.reshape(-1), minlength=n_g + 1)
            vd = np.bincount(pl.reshape(-1)[is_void.reshape(-1)], minlength=n_p + 1)
            keys, inter = np.unique(gl.reshape(-1).astype(np.int64) * (n_p + 1) + pl.reshape(-1), return_counts=True)
            g, q = keys // (n_p + 1), keys % (n_p + 1)
            ok = (g > 0) & (q > 0)
            g, q, inter = g[ok], q[ok], inter[ok]
            hit = 2 * inter > pa[q] - vd[q] + ga[g] - inter
            matched = np.zeros(n_p + 1, dtype=bool)
            matched[q[hit]] = True
            tp = int(hit.sum())
            tally[k, c] = (tp, int((~matched[1:] & (2 * vd[1:] <= pa[1:])).sum()), n_g - tp)
    return tally


def kernel_rates(dev, reps, only_map, only_shape, torch_form, host):
    from vq_seg_amd import _hip, nnf
    from vq_seg_amd.utils import instances
    L = _hip.lib()
    out = {}
    for b, h, w in (SHAPES if only_shape < 0 else SHAPES[only_shape:only_shape + 1]):
        px = b * h * w
        for kind, make in (("blobs, shifted by 3", blob_pair), ("random", random_pair), ("one value", constant_pair)):
            if only_map and only_map not in kind:
                continue
            p, t = make(dev, b, h, w)
            cap = MAX_CAPACITY if kind == "random" else CAPACITY
            rows = {"capacity": cap}
            sides = []
            for m in (p, t):
                tm, ign = instances._things_only(m, (1, 2), False)
                roots = nnf.region_roots(tm, 4, (ign,))
                ids, counts = nnf.region_ids(roots)
                table, _mom = nnf.region_table(tm, roots, ids, counts, cap)
                sides.append((roots, ids, counts, table))
            (proots, pid, pc, ptab), (_groots, gid, gc, gtab) = sides
            rows["regions per image (prediction, ground truth)"] = [[int(pc.min()), int(pc.max())], [int(gc.min()), int(gc.max())]]
            nb = int(L.vqseg_instance_vote_bits(cap))
            votes = torch.empty((b, cap, nb), dtype=torch.int32, device=dev)
            void, cand, inter, match, union, matched = (torch.empty((b, cap), dtype=torch.int32, device=dev) for _ in range(6))
            tally = torch.empty((b, C, 5), dtype=torch.int32, device=dev)
            iou = torch.empty((b, C), dtype=torch.float64, device=dev)
            over = torch.empty((b,), dtype=torch.int32, device=dev)
            P = lambda x: x.data_ptr()
            vote = lambda: _hip.launch("vqseg_instance_vote_i32", dev, P(pid), P(gid), P(t), 1, b, h, w, cap, 1, 255, 0, 0, 0, P(votes), P(void))
            overlap = lambda: _hip.launch("vqseg_instance_overlap_i32", dev, P(pid), P(gid), P(votes), P(gtab), b, h, w, cap, P(cand), P(inter))
            keep = torch.empty_like(inter)

            def match_():
                inter.copy_(keep)                             # the match launch rewrites inter: every repetition starts from the overlap's
                _hip.launch("vqseg_instance_match_i32", dev, P(cand), P(void), P(ptab), P(gtab), P(pc), P(gc), b, cap, P(inter), P(match), P(union),
                            P(matched))
            tally_ = lambda: _hip.launch("vqseg_instance_tally_i32", dev, P(match), P(matched), P(inter), P(union), P(void), P(ptab), P(gtab), P(pc),
                                         P(gc), b, cap, C, P(tally), P(iou), P(over))
            areas = lambda: nnf.region_areas(proots)
            rows["region_areas (the yardstick)"] = _row(*_time(areas, reps), px * 4)
            rows["vote"] = _row(*_time(vote, reps), px * 8)
            rows["overlap"] = _row(*_time(overlap, reps), px * 8)
            keep.copy_(inter)
            med, mn = _time(match_, reps)
            rows["match (with a copy of inter)"] = {"us": round(med, 1), "us_min": round(mn, 1)}
            med, mn = _time(tally_, reps)
            rows["tally"] = {"us": round(med, 1), "us_min": round(mn, 1)}
            per_byte = rows["region_areas (the yardstick)"]["us"] / (px * 4)
            for key in ("vote", "overlap"):
                rows[key]["time per byte over region_areas'"] = round(rows[key]["us"] / (px * 8) / per_byte, 2)
            kw = dict(capacity=cap)
            rows["panoptic_stats"] = _row(*_time(lambda: instances.panoptic_stats(p, t, C, **kw), reps), px * 111)
            want = instances.panoptic_stats(p, t, C, **kw)
            assert torch.equal(tally, want.table) and torch.equal(over, want.overflow) and torch.equal(iou, want.iou_sum), \
                "the launches on their own differ from panoptic_stats"
            rows["images that overflow"] = int(want.overflow.sum())
            rows["result"] = {"pq": want.pq, "sq": want.sq, "rq": want.rq, "count_error": want.count_error,
                              "tp, fp, fn": want.table[:, :, :3].sum(dim=(0, 1)).tolist()}
            if torch_form:
                sides_t = [(s[1], s[2], s[3]) for s in sides]
                form = lambda: instances.overlap_torch(sides_t[0][0], sides_t[1][0], t, sides_t[0][2], sides_t[1][2], sides_t[0][1], sides_t[1][1],
                                                       (255,), cap, C)
                form()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r, _v = form()
                torch.cuda.synchronize()
                rows["torch ops: overlap + matching + tally from the same ids"] = {"us": round((time.perf_counter() - t0) * 1e6, 1), "runs": 1}
                assert torch.equal(r.tally, want.table) and torch.equal(r.iou_sum, want.iou_sum), "torch-op tables differ from the kernels'"
            if host:
                t0 = time.perf_counter()
                got = host_form(p, t)
                rows["numpy / scipy on the host, copies included"] = {"us": round((time.perf_counter() - t0) * 1e6, 1), "runs": 1}
                if not int(want.overflow.sum()):
                    assert np.array_equal(got, want.table[:, :, :3].cpu().numpy()), "the host form's counts differ from the kernels'"
            out[f"{b} x {h} x {w}, {kind}"] = rows
            print(f"bench_instances: {b} x {h} x {w}, {kind} done", file=sys.stderr, flush=True)
            del votes, void, cand, inter, match, union, matched, keep, sides, p, t
            torch.cuda.empty_cache()
    return {"classes": C, "things": [1, 2], "connectivity": 4, "note": "events around the entry points on buffers made once (panoptic_stats and "
            "the torch-op form: around the Python call); GB/s are the bytes the pass must read over the time", "rows": out}


def loop_times(dev, reps):
    """evaluate.test_loop(fused=True) on the cfg3 network over two synthetic batches, with and without panoptic=True"""
    import bench
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    wl = bench.WORKLOADS["cfg3"]
    data = SyntheticCropWeed(wl["size"], wl["batch"], dev, seed=42)
    batches = [data.labelled() for _ in range(2)]
    tr = CPSTrainer(CPSConfig(model=bench.model_cfg("cfg3"), recipe="v1", total_iters=16, amp_dtype=torch.bfloat16), dev)
    rows = {}
    for key, kw in (("fused", {}), ("fused, panoptic=True", dict(panoptic=True))):
        times = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = tr.evaluate(batches, fused=True, **kw)
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        rows[key] = {"ms": round(statistics.median(times), 2), "ms_min": round(min(times), 2),
                     "result": {k: v for k, v in res.items() if k in ("test_miou", "test_pq", "test_sq", "test_rq", "test_count_error", "test_panoptic_overflowed")}}
    return {"shape": list(batches[0][0].shape), "batches": len(batches), "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", type=int, default=-1, help="only this entry of SHAPES")
    ap.add_argument("--map", default="", help="only the inputs whose name contains this")
    ap.add_argument("--no-torch-form", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_instances: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {} if args.no_kernel else {"kernel": kernel_rates(dev, args.reps, args.map, args.shape, not args.no_torch_form, not args.no_host)}
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
