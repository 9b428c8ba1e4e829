"""What feeding the CPS step from an image folder costs: the benchmark's step (cfg3: vqreptunet1x1, 512 x 512, K = 512, bf16,
32 labelled + 32 unlabelled images, CPSTrainer) driven by the reference's loop (train_vqreptunet1x1v2.py:89-90,118,130-139:
zip(cycle(sup_loader), unsup_loader), img_to_label, .to(device)) over a synthetic folder of CWFID-sized 1296 x 966 PNGs, fed by

    synthetic   tensors already in HBM (data.synthetic.SyntheticCropWeed, what bench.py times)
    device      vq_seg_amd.data.DeviceLoader (cache built once; one assembly kernel per batch)
    workers     DataLoader(BaseDataset, num_workers=...): min(16, CPUs of this process) workers in all, half per loader
                (spawned processes; persistent across epochs)
    reference   DataLoader(BaseDataset) with num_workers=0, the reference's loop as written

Per leg: images/s over the timed steps (host clock, the device synchronised at the end) and the mean host time per step spent
waiting for the batch (next() + img_to_label + .to(device)); for `device` also the one-time cache build.  Every leg runs one
untimed step first.  One JSON line per leg, and with --out a JSON file of all of them.

    python tools/bench_data_path.py [--steps 20] [--workers-steps 6] [--ref-steps 2] [--legs synthetic,device,workers,reference]
                                    [--data DIR] [--out F]          (a leg named twice runs twice: same-box spread)
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P2L = {"0": 0, "128": 1, "255": 2}            # config/vqreptunet1x1.json pixel_to_label
SRC_W, SRC_H = 1296, 966                      # CWFID's image size


def assembly_bytes(batch: int, size: int) -> dict:
    """HBM bytes the assembly kernel must move per step (B labelled + B unlabelled): u8 images read, f32 images written, masks read +
    written, int64 labels written."""
    px = batch * size * size
    d = {"img_u8_read": 2 * 3 * px, "img_f32_written": 2 * 3 * px * 4, "mask_read": px, "mask_written": px, "label_written": 8 * px}
    d["total"] = sum(d.values())
    return d


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20, help="timed steps of the synthetic / device legs")
    ap.add_argument("--workers-steps", type=int, default=6, help="timed steps of the workers leg")
    ap.add_argument("--ref-steps", type=int, default=2, help="timed steps of the reference leg (seconds each)")
    ap.add_argument("--legs", default="synthetic,device,workers,reference")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--n-labelled", type=int, default=32)
    ap.add_argument("--n-unlabelled", type=int, default=64)
    ap.add_argument("--data", default="", help="dataset folder (written if it has no input/ yet); default: a temporary one")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch
    from torch.utils.data import DataLoader

    import bench
    from vq_seg_amd.data import BaseDataset, DeviceLoader, write_synthetic_dataset
    from vq_seg_amd.data.device_loader import loader_threads
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    from vq_seg_amd.utils.seg_tools import img_to_label

    assert torch.cuda.is_available(), "bench_data_path.py measures on the GPU; there is no CPU mode"
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    tmp = None
    data = args.data
    if not data:
        tmp = tempfile.TemporaryDirectory(prefix="vqseg_data_")
        data = tmp.name
    if not os.path.isdir(os.path.join(data, "input")):
        t0 = time.perf_counter()
        write_synthetic_dataset(data, args.n_labelled, args.n_unlabelled, size=(SRC_W, SRC_H), seed=0, cell=32)
        print(f"[data] wrote {args.n_labelled} + {args.n_unlabelled} {SRC_W}x{SRC_H} PNGs in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    sup_ds = BaseDataset(data, split="labelled", batch_size=B, resize=S)
    unsup_ds = BaseDataset(data, split="unlabelled", batch_size=B, resize=S)

    trainer = CPSTrainer(CPSConfig(model=bench.model_cfg("cfg3"), recipe="v1", total_iters=10 ** 6, amp_dtype=torch.bfloat16), dev)
    syn = SyntheticCropWeed(S, B, dev, seed=42)
    syn_batches = [(syn.labelled(), syn.unlabelled()) for _ in range(2)]
    for i in range(2):                                                   # warm-up: code objects, allocator
        (l_in, l_tg), ul = syn_batches[i]
        trainer.step(l_in, l_tg, ul)
    torch.cuda.synchronize()

    def epochs(sup_loader, unsup_loader):
        while True:
            for pair in zip(itertools.cycle(sup_loader), unsup_loader):
                yield pair

    def run_leg(name, batches, fetch, steps, extra=None):
        """batches: iterator of raw batches; fetch(raw) -> (l_input, l_target, ul_input) on the device."""
        waits = []
        for i in range(steps + 1):
            if i == 1:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            tw = time.perf_counter()
            l_in, l_tg, ul = fetch(next(batches))
            if i >= 1:
                waits.append(time.perf_counter() - tw)
            trainer.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        rec = {"leg": name, "steps": steps, "batch": f"{B}+{B}", "size": S, "images_per_s": round(2 * B * steps / el, 2),
               "ms_per_step": round(1e3 * el / steps, 2), "data_wait_ms_per_step": round(1e3 * sum(waits) / steps, 3)}
        rec.update(extra or {})
        print(json.dumps(rec), flush=True)
        return rec

    legs = [x for x in args.legs.split(",") if x]
    results = []
    for leg in legs:
        if leg == "synthetic":
            it = itertools.cycle(syn_batches)
            results.append(run_leg(leg, it, lambda b: (b[0][0], b[0][1], b[1]), args.steps))
        elif leg == "device":
            sup = DeviceLoader(sup_ds, batch_size=B, shuffle=True, device=dev, pixel_to_label=P2L)
            unsup = DeviceLoader(unsup_ds, batch_size=B, shuffle=True, device=dev)
            extra = {"cache_build_s": round(sup.build_seconds + unsup.build_seconds, 3), "cache_bytes": sup.cache_bytes + unsup.cache_bytes,
                     "loader_threads": loader_threads(), "assembly_bytes_per_step": assembly_bytes(B, S)["total"]}
            results.append(run_leg(leg, epochs(sup, unsup), lambda b: (b[0]["img"], b[0]["label"], b[1]["img"]), args.steps, extra))
            del sup, unsup
        elif leg in ("workers", "reference"):
            nw = loader_threads() // 2 if leg == "workers" else 0
            kw = dict(num_workers=nw, multiprocessing_context="spawn", persistent_workers=True) if nw else {}
            sup = DataLoader(sup_ds, batch_size=B, shuffle=True, **kw)
            unsup = DataLoader(unsup_ds, batch_size=B, shuffle=True, **kw)

            def fetch(b):                                                # train_vqreptunet1x1v2.py:130-139
                return b[0]["img"].to(dev), img_to_label(b[0]["target"], P2L).to(dev), b[1]["img"].to(dev)

            steps = args.workers_steps if leg == "workers" else args.ref_steps
            results.append(run_leg(leg, epochs(sup, unsup), fetch, steps, {"num_workers_per_loader": nw}))
            del sup, unsup
        else:
            raise SystemExit(f"unknown leg {leg!r}")
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"legs": results, "source_png": [SRC_W, SRC_H], "files": [args.n_labelled, args.n_unlabelled],
                       "assembly_bytes_per_step": assembly_bytes(B, S)}, f, indent=1)
    if tmp is not None:
        tmp.cleanup()


if __name__ == "__main__":
    main()
