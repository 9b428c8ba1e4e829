"""Tiled-prediction cost (profiles/tiled_predict.md): the two launches around the forwards of predict.Predictor(window=...) at CWFID's
native size -- 4 x 3 x 966 x 1296 images, 512 x 512 windows at stride 256 (3 x 5 windows per image), the "linear" blend, 1 and 4 views:

  * nnf.extract_windows (vqseg_extract_windows_f): all windows of all flips in one launch;
  * nnf.merge_argmax (vqseg_merge_argmax_f, label + counts) next to the same result from torch device ops in the SAME process --
    accumulate w * logits and w per window into (B, C, H, W) / (H, W), divide, average the views, then nnf.softmax_stats and
    measurement.confusion_matrix_device;
  * Predictor end to end with a real vqreptunet1x1 (bench.py's cfg3, bf16 autocast): tiled against today's path (the image squeezed
    to 512 x 512, the logits stretched back by nnf.resize_argmax).

All arms of a group in ONE process, timed in interleaved rounds with device events around `reps` back-to-back calls of the Python
wrapper: the times, and the GB/s derived from them, include the wrapper's host work where the device waits for it, and are not
kernel-trace times.

    python tools/bench_tiled_predict.py [--rounds 7] [--reps 20] [--no-model] [--out FILE] [--md FILE]

Bytes are what each launch must move, computed from the shapes: extract reads each image once (the overlap is served by the caches)
and writes F * B * T * 3 * nh * nw floats; merge reads every view's window logits once and the 8-byte target and writes the 1-byte label.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, SIZE, WINDOW, STRIDE, CLASSES = 4, (966, 1296), (512, 512), (256, 256), 3
FLIPS = {1: [0], 4: [0, 1, 2, 3]}


def timed(arms, rounds, reps):
    """{name: (fn, bytes | None)} -> {name: stats}: three warm-up calls each, then interleaved rounds (order reversed every other
    round) of `reps` calls between two device events"""
    for fn, _ in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms, keys = {k: [] for k in arms}, list(arms)
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                arms[key][0]()
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / reps)
    out = {}
    for key, vs in ms.items():
        med, nbytes = statistics.median(vs), arms[key][1]
        out[key] = {"us_median": round(med * 1e3, 1), "us_min": round(min(vs) * 1e3, 1), "us_max": round(max(vs) * 1e3, 1)}
        if nbytes is not None:
            out[key].update(bytes=nbytes, GB_per_s=round(nbytes / med / 1e6, 1))
    return out


def merge_with_torch_ops(views, flips, grid, target):
    """what nnf.merge_argmax replaces, with device ops: -> (label i64, counts)"""
    from vq_seg_amd import nnf
    from vq_seg_amd.measurement import confusion_matrix_device
    (wh, ww), c = grid.window, views[0].shape[1]
    dev = views[0].device
    ry, rx = torch.arange(wh, dtype=torch.float32, device=dev), torch.arange(ww, dtype=torch.float32, device=dev)
    w = torch.minimum(ry + 1, wh - ry)[:, None] * torch.minimum(rx + 1, ww - rx)[None, :]
    ys, xs = nnf.window_starts(grid.height, wh, grid.stride[0]), nnf.window_starts(grid.width, ww, grid.stride[1])
    ws = torch.zeros((grid.height, grid.width), dtype=torch.float32, device=dev)
    for y0 in ys:
        for x0 in xs:
            ws[y0:y0 + wh, x0:x0 + ww] += w
    z = None
    for v, f in zip(views, flips):
        s = (v.flip(nnf.FLIP_DIMS[f]) if f else v).reshape(grid.batch, grid.ny * grid.nx, c, wh, ww)
        acc = torch.zeros((grid.batch, c, grid.height, grid.width), dtype=torch.float32, device=dev)
        for j, y0 in enumerate(ys):
            for i, x0 in enumerate(xs):
                acc[:, :, y0:y0 + wh, x0:x0 + ww].addcmul_(s[:, j * grid.nx + i], w)
        m = acc / ws
        z = m if z is None else z + m
    if len(views) > 1:
        z = z * (1.0 / len(views))
    label = nnf.softmax_stats(z, want_label=True, want_entropy=False, want_top=False)[0]
    return label, confusion_matrix_device(z, target, c)


def launches(dev, rounds, reps):
    from vq_seg_amd import nnf
    g = torch.Generator().manual_seed(0)
    images = torch.rand((BATCH, 3) + SIZE, generator=g).to(dev)
    target = torch.randint(0, CLASSES, (BATCH,) + SIZE, generator=g).to(dev)
    out = {}
    arms = {}
    for n, flips in FLIPS.items():
        _w, grid = nnf.extract_windows(images, WINDOW, STRIDE, flips=flips)
        rows = BATCH * grid.ny * grid.nx
        nbytes = images.numel() * 4 + n * rows * 3 * WINDOW[0] * WINDOW[1] * 4
        arms[f"extract: {n} flip{'s' if n > 1 else ''}"] = (lambda flips=flips: nnf.extract_windows(images, WINDOW, STRIDE, flips=flips), nbytes)
        del _w
    out.update(timed(arms, rounds, reps))
    px = BATCH * SIZE[0] * SIZE[1]
    for n, flips in FLIPS.items():
        views = [(torch.randn((rows, CLASSES) + WINDOW, generator=g) * 4.0).to(dev) for _ in range(n)]
        fused = nnf.merge_argmax(views, grid, flips=flips, target=target)
        label, counts = merge_with_torch_ops(views, flips, grid, target)
        differ = int((fused[0].long() != label).sum())
        nbytes = n * views[0].numel() * 4 + px * 9
        arms = {f"merge, {n} view{'s' if n > 1 else ''}: kernel": (lambda: nnf.merge_argmax(views, grid, flips=flips, target=target), nbytes),
                f"merge, {n} view{'s' if n > 1 else ''}: torch ops": (lambda: merge_with_torch_ops(views, flips, grid, target), None)}
        out.update(timed(arms, rounds, reps))
        out[f"merge, {n} view{'s' if n > 1 else ''}: labels that differ from the torch ops'"] = f"{differ} of {px}"
        del views, fused, label, counts
    return out


def end_to_end(dev, rounds):
    import bench
    from vq_seg_amd.models.networks import make_model
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.trainer import SyntheticCropWeed
    torch.manual_seed(0)
    model = make_model(bench.model_cfg("cfg3")).to(dev)
    big = SyntheticCropWeed(1296, BATCH, dev, seed=42).labelled()[0][:, :, :SIZE[0]].contiguous()
    tiled = Predictor(model, CLASSES, amp_dtype=torch.bfloat16, window=WINDOW, stride=STRIDE, window_batch=BATCH * 5)
    plain = Predictor(model, CLASSES, amp_dtype=torch.bfloat16)

    def resized():
        small = torch.nn.functional.interpolate(big, size=WINDOW, mode="bilinear", align_corners=False)
        return plain(small, size=SIZE)

    arms = {"Predictor: tiled (60 windows of 512 x 512, chunks of 20)": (lambda: tiled(big), None),
            "Predictor: resized (4 images squeezed to 512 x 512)": (resized, None)}
    out = timed(arms, rounds, 3)
    agree = (tiled(big).label == resized().label).float().mean().item()
    out["Predictor: share of pixels where the two agree (untrained network)"] = round(agree, 4)
    return out


def markdown(res):
    lines = ["| case | us (median) | us (min .. max) | bytes | GB/s |", "|---|---|---|---|---|"]
    notes = []
    for k, v in res.items():
        if isinstance(v, dict):
            lines.append(f"| {k} | {v['us_median']} | {v['us_min']} .. {v['us_max']} | {v.get('bytes', '')} | {v.get('GB_per_s', '')} |")
        else:
            notes.append(f"{k}: {v}")
    return "\n".join(lines + [""] + notes) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled_predict: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = launches(dev, args.rounds, args.reps)
    if not args.no_model:
        res.update(end_to_end(dev, max(args.rounds // 2, 2)))
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
