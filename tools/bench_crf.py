"""Dense-CRF cost (profiles/crf.md): the two launches of nnf.dense_crf at the reference's default settings (bi_xy_std 50 and
pos_xy_std 3 under truncate 4: supports of 401 x 401 and 25 x 25 pixels), C = 3:

  * vqseg_crf_prepare_f (colours, unary, Q0, both norms: the bilateral norm is an all-pairs pass of its own) and ONE
    vqseg_crf_step_f launch, at 512 x 512 and 966 x 1296 with B = 1 and B = 4;
  * the same update as chunked torch device ops (utils.crf.mean_field_torch on GPU tensors, float32) at a size where that form
    fits, next to the kernel at that size;
  * Predictor end to end with a real vqreptunet1x1 (bench.py's cfg3, bf16 autocast) with and without crf.

Pairs are counted from the shapes: sum over the pixels i of the pixels j inside the support, cut at the image, per kernel.  Each
pair costs one v_exp_f32; the exp issue peak is 256 CUs x 4 SIMDs x 16 lanes per clock (a wave's v_exp_f32 issues over 4 cycles when
other waves fill the gaps) at 2.4 GHz = 3.93e13 per second, and the share reported is (pairs of both kernels) / time over that peak.
It counts the pairs of the contract, not the tile overhang the kernel also walks.

All arms of a group in ONE process, timed in interleaved rounds with device events around back-to-back calls of the Python wrapper;
the times include the wrapper's host work where the device waits for it and are not kernel-trace times.

    python tools/bench_crf.py [--rounds 5] [--no-model] [--out FILE] [--md FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = 3
SHAPES = [(1, 512, 512), (4, 512, 512), (1, 966, 1296), (4, 966, 1296)]
TORCH_OPS_SHAPE = (1, 128, 160)                 # the chunked torch-op form holds (rows x window) blocks: minutes at 512 x 512
EXP_PEAK = 256 * 4 * 16 * 2.4e9


def pairs_in_support(h, w, r):
    """sum over i of |{j: |dx| <= r, |dy| <= r}| inside an h x w image (separable)"""
    def axis(n):
        return sum(min(n - 1, k + r) - max(0, k - r) + 1 for k in range(n))
    return axis(h) * axis(w)


def timed(arms, rounds, reps):
    """{name: fn} -> {name: ms median / min / max}: two warm-up calls each, then interleaved rounds of `reps` calls between events"""
    for fn in arms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms, keys = {k: [] for k in arms}, list(arms)
    for r in range(rounds):
        for key in (keys if r % 2 == 0 else keys[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                arms[key]()
            e1.record()
            e1.synchronize()
            ms[key].append(e0.elapsed_time(e1) / reps)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def inputs(b, h, w, dev, seed=0):
    from vq_seg_amd.trainer import SyntheticCropWeed
    side = max(h, w)
    x, lab = SyntheticCropWeed(side, b, dev, seed=seed).labelled()
    x, lab = x[:, :, :h, :w].contiguous(), lab[:, :h, :w]
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((b, CLASSES, h, w), generator=g).to(dev) + 1.5 * torch.nn.functional.one_hot(lab.clamp(0, CLASSES - 1), CLASSES).permute(0, 3, 1, 2)
    return x, torch.softmax(logits, dim=1)


def launches(dev, rounds):
    from vq_seg_amd import nnf
    s = nnf.crf_settings()
    iters, bi_w, bi_xy, bi_rgb, pos_w, pos_xy, trunc = s
    rb, rp = int(-(-trunc * bi_xy // 1)), int(-(-trunc * pos_xy // 1))
    out = {}
    for b, h, w in SHAPES:
        x, p = inputs(b, h, w, dev)
        state = nnf._crf_prepare(x, p, iters, bi_xy, bi_rgb, pos_xy, trunc)
        arms = {"prepare": lambda: nnf._crf_prepare(x, p, iters, bi_xy, bi_rgb, pos_xy, trunc),
                "step": lambda: nnf._crf_step(state, 0, bi_w, bi_xy, bi_rgb, pos_w, pos_xy, trunc, False)}
        t = timed(arms, rounds, 2 if b * h * w > 1 << 20 else 5)
        n_bi, n_pos = b * pairs_in_support(h, w, rb), b * pairs_in_support(h, w, rp)
        step_s = t["step"][0] * 1e-3
        out[f"B={b} {h}x{w}"] = {
            "prepare_us": round(t["prepare"][0] * 1e3, 1), "prepare_us_min_max": [round(t["prepare"][1] * 1e3, 1), round(t["prepare"][2] * 1e3, 1)],
            "step_us": round(t["step"][0] * 1e3, 1), "step_us_min_max": [round(t["step"][1] * 1e3, 1), round(t["step"][2] * 1e3, 1)],
            "bilateral_pairs": n_bi, "positional_pairs": n_pos, "pairs_per_s": round((n_bi + n_pos) / step_s, 0),
            "share_of_exp_issue_peak": round((n_bi + n_pos) / step_s / EXP_PEAK, 4)}
        del state, x, p
    return out


def torch_ops(dev, rounds):
    """one update with chunked torch device ops against the kernel at the same size (ten updates each, per-update time reported)"""
    from vq_seg_amd import nnf
    from vq_seg_amd.utils.crf import mean_field_torch
    b, h, w = TORCH_OPS_SHAPE
    x, p = inputs(b, h, w, dev, seed=1)
    arms = {"kernel": lambda: nnf.dense_crf(x, p), "torch ops": lambda: mean_field_torch(x[0], p[0], dtype=torch.float32)}
    t = timed(arms, rounds, 1)
    q_k, q_t = nnf.dense_crf(x, p)[0], mean_field_torch(x[0], p[0], dtype=torch.float32)[0]
    return {f"B={b} {h}x{w}, 10 updates + norms": {
        "kernel_us": round(t["kernel"][0] * 1e3, 1), "torch_ops_us": round(t["torch ops"][0] * 1e3, 1),
        "max_abs_difference_of_Q": float((q_k - q_t).abs().max())}}


def end_to_end(dev, rounds):
    import bench
    from vq_seg_amd.models.networks import make_model
    from vq_seg_amd.predict import Predictor
    torch.manual_seed(0)
    model = make_model(bench.model_cfg("cfg3")).to(dev)
    x, _ = inputs(4, 512, 512, dev, seed=2)
    plain, refined = Predictor(model, CLASSES, amp_dtype=torch.bfloat16), Predictor(model, CLASSES, amp_dtype=torch.bfloat16, crf=True)
    t = timed({"plain": lambda: plain(x), "crf": lambda: refined(x)}, rounds, 1)
    moved = (plain(x).label != refined(x).label).float().mean().item()
    return {"Predictor B=4 512x512": {"plain_us": round(t["plain"][0] * 1e3, 1), "crf_us": round(t["crf"][0] * 1e3, 1),
                                      "share_of_labels_the_crf_moves (untrained network)": round(moved, 4)}}


def markdown(res):
    lines = []
    for group, rows in res.items():
        lines.append(f"**{group}**\n")
        for k, v in rows.items():
            lines.append(f"* {k}: " + ", ".join(f"{a} = {b}" for a, b in v.items()))
        lines.append("")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crf: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    res = {"launches (defaults, C=3)": launches(dev, args.rounds), "torch device ops": torch_ops(dev, max(args.rounds // 2, 2))}
    if not args.no_model:
        res["end to end"] = end_to_end(dev, max(args.rounds // 2, 2))
    line = json.dumps(res)
    print(line)
    for path, text in ((args.out, line + "\n"), (args.md, markdown(res))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
