"""Visualisation-path cost (profiles/visualize.md): the panel-sheet kernel (nnf.render_sheet, vqseg_render_sheet_u8) on the flagship
batch -- 32 x 3 x 512 x 512 images, labels and targets at 512 x 512 -> the five-panel sheet [image | target | pred | 20 px | mix], full size
and halved -- next to (a) the same sheet composed from torch device ops and (b) the reference-arithmetic numpy path of
utils.visualize including the device-to-host copies it needs.  All arms in ONE process, timed in interleaved rounds; the device arms
with device events, the host arms (which end on the host) with a wall clock around a synchronised call.

    python tools/bench_visualize.py [--rounds 7] [--reps 10] [--host-rounds 2] [--out FILE] [--md FILE]

Bytes are what the kernel must move, computed from the shapes: the sheet's bytes written (3 per pixel) plus every source read once
(image 12 bytes per pixel, label 1, target 8); the second panel that reads a source is served by the caches.
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

PANELS = ["image", "target", "pred", ("fill", 20), "mix_pred"]


def torch_sheet(image, label, target, pal, half, alpha=0.4):
    """baseline (a): the same bytes from torch device ops (identity display size: no resize needed)"""
    b, _, h, w = image.shape
    img = image.permute(0, 2, 3, 1).reshape(b * h, w, 3)
    tgt = pal[target.reshape(b * h, w)]
    prd = pal[label.reshape(b * h, w).long()]
    mix = (img * (1 - alpha) + prd * alpha).clamp(0, 1)
    sheet = torch.cat([img, tgt, prd, torch.ones((b * h, 20, 3), device=image.device), mix], dim=1)
    if half:
        sheet = torch.nn.functional.avg_pool2d(sheet.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0)
    return (sheet.clamp(0, 1) * 255).floor().to(torch.uint8)


def measure(dev, batch, src, rounds, reps, host_rounds):
    from vq_seg_amd import nnf
    from vq_seg_amd.utils import visualize as V
    from vq_seg_amd.utils.processing import detach_numpy
    g = torch.Generator().manual_seed(0)
    image = torch.rand((batch, 3, src, src), generator=g).to(dev).contiguous(memory_format=torch.channels_last)      # as DeviceLoader hands it over
    logits = (torch.randn((batch, 3, src, src), generator=g) * 4.0).to(dev)
    target = torch.randint(0, 3, (batch, src, src), generator=g).to(dev)
    size = (src, src)
    label = nnf.resize_argmax(logits, size)[0]
    pal64 = V.default_palette(3)
    pal = torch.tensor(pal64, dtype=torch.float32, device=dev)
    rows, cols = batch * src, 4 * src + 20
    canvas = {False: torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev), True: torch.empty((rows // 2, cols // 2, 3), dtype=torch.uint8, device=dev)}
    px = batch * src * src
    sources = px * (12 + 1 + 8)
    dev_arms, res = {}, {}
    for half in (False, True):
        tag = "half" if half else "full"
        sheet_bytes = canvas[half].numel()
        dev_arms[f"{tag}: kernel"] = (lambda half=half: nnf.render_sheet(PANELS, size, 3, pal64, image=image, pred=label, target=target, half=half,
                                                                         out=canvas[half]), sheet_bytes + sources)
        dev_arms[f"{tag}: torch device ops"] = (lambda half=half: torch_sheet(image, label, target, pal, half), sheet_bytes + sources)
        got = dev_arms[f"{tag}: kernel"][0]().clone()
        ref = dev_arms[f"{tag}: torch device ops"][0]()
        diff = (got.int() - ref.int()).abs()
        res[f"{tag}: kernel vs torch ops, bytes that differ"] = f"{int((diff > 0).sum())} of {got.numel()} (largest difference {int(diff.max())})"
        del got, ref, diff
    for fn, _ in dev_arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in dev_arms}
    keys = list(dev_arms)
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            fn = dev_arms[key][0]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / reps)
    for key, vs in ms.items():
        med, nbytes = statistics.median(vs), dev_arms[key][1]
        res[f"{batch}x3x{src}x{src} five panels {key}"] = {"bytes": nbytes, "us_median": round(med * 1e3, 1), "us_min": round(min(vs) * 1e3, 1),
                                                           "us_max": round(max(vs) * 1e3, 1), "GB_per_s": round(nbytes / med / 1e6, 1)}
    # end to end, host array in hand: the device path of make_example_img (arg-max of both logit tensors, two launches, the sheet's
    # bytes over PCIe) against the numpy path on arrays copied off the device first, as the reference trainer does
    host_arms = {
        "make_example_img: device tensors (kernel path, sheet copied to the host)":
            lambda f: V.make_example_img(image, target, logits, image, logits, resize_factor=f),
        "make_example_img: detach_numpy first (numpy path, reference arithmetic)":
            lambda f: V.make_example_img(*[detach_numpy(t) for t in (image, target, logits, image, logits)], resize_factor=f),
    }
    for f, tag in ((None, "full"), (0.5, "half")):
        outs = {k: fn(f) for k, fn in host_arms.items()}               # warm-up, and the two results
        a, b = list(outs.values())
        diff = np.abs(a.astype(np.int64) - b.astype(np.int64))
        res[f"{tag}: device path vs numpy path, bytes that differ"] = f"{int((diff > 0).sum())} of {a.size} (largest difference {int(diff.max())})"
        hms = {k: [] for k in host_arms}
        hkeys = list(host_arms)
        for r in range(host_rounds):
            for key in (hkeys if r % 2 == 0 else hkeys[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_arms[key](f)
                torch.cuda.synchronize()
                hms[key].append((time.perf_counter() - t0) * 1e3)
        for key, vs in hms.items():
            res[f"{batch}x3x{src}x{src} {tag} {key}"] = {"ms_median": round(statistics.median(vs), 2), "ms_min": round(min(vs), 2), "ms_max": round(max(vs), 2)}
    return res


def markdown(res):
    lines = ["| case | bytes | us (median) | us (min .. max) | GB/s |", "|---|---|---|---|---|"]
    lines += [f"| {k} | {v['bytes']} | {v['us_median']} | {v['us_min']} .. {v['us_max']} | {v['GB_per_s']} |" for k, v in res.items()
              if isinstance(v, dict) and "bytes" in v]
    lines += ["", "| case | ms (median) | min .. max |", "|---|---|---|"]
    lines += [f"| {k} | {v['ms_median']} | {v['ms_min']} .. {v['ms_max']} |" for k, v in res.items() if isinstance(v, dict) and "ms_median" in v]
    lines += [""] + [f"{k}: {v}" for k, v in res.items() if not isinstance(v, dict)]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src", type=int, default=512)
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visualize: needs a GPU (nothing is measured without one)")
    res = measure(torch.device("cuda:0"), args.batch, args.src, args.rounds, args.reps, args.host_rounds)
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
