"""Micro-benchmark of the VQ kernels on one MI355X (not the headline bench; see bench.py).
    python tools/bench_vq.py [B]        each level alone, fp32 rows
    python tools/bench_vq.py s3 [B]     the grouped launch of the three bench levels on split-3 rows (the pseudo-label forwards' VQ phase):
                                        candidate filter against the exact kernel, against the earlier merge -> exact -> gather -> split
                                        path, candidate pairs per row; once on a k-means-separated codebook, once on the untrained
                                        network's own eval features (what the bench step feeds it)"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vq_seg_amd import _hip  # noqa: E402


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    dev = torch.device("cuda:0")
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    print(torch.cuda.get_device_name(0), "B =", B)
    for name, n, c, k in [("L2 512^2", B * 4096, 512, 512), ("L3 512^2", B * 1024, 1024, 512),
                          ("L4 512^2", B * 256, 2048, 512), ("L2 K=256", B * 4096, 512, 256),
                          ("L2 1024^2 K=1024", B * 16384 // 4, 512, 1024)]:
        x = torch.relu(torch.randn(n, c, device=dev))
        W = torch.relu(torch.randn(k, c, device=dev))
        prep = _hip.vq_prepare(W)
        t_as = timeit(lambda: _hip.vq_assign(x, W, prepared=prep))
        t_fw = timeit(lambda: _hip.vq_forward(x, W, True, 1.0, prepared=prep))
        flops = 2.0 * n * k * c
        byts = n * (c * 4 * 2 + 8)
        print(f"{name:18s} N={n:7d} C={c:4d} K={k:4d}  assign {t_as*1e3:8.1f} us  {flops/t_as/1e9:7.1f} TF/s "
              f"({flops/t_as/1e9/157.3*100:4.1f}% of 157.3)   forward {t_fw*1e3:8.1f} us  alg {byts/t_fw/1e6:7.1f} GB/s")


def s3_split(x):
    n, c = x.shape
    y = torch.empty((n, 2 * c), dtype=torch.bfloat16, device=x.device)
    _hip.launch("vqseg_s3_split_f", x.device, _hip.tptr(x, "rows", dtype=torch.float32, numel=n * c), n, c, _hip.tptr(y, "split-3 rows", bf=2, numel=2 * n * c))
    return y


def s3_merge(y):
    n, c2 = y.shape
    x = torch.empty((n, c2 // 2), dtype=torch.float32, device=y.device)
    _hip.launch("vqseg_s3_merge_f", y.device, _hip.tptr(y, "split-3 rows", bf=2, numel=n * c2), n, c2 // 2, _hip.tptr(x, "rows", dtype=torch.float32, numel=n * c2 // 2))
    return x


def s3_arm(name, rows_s3, books, reps=5):
    """rows_s3: the three levels' split-3 rows (N, 2C); every timing is the median of `reps` event-timed runs of 10 calls"""
    preps = [_hip.vq_prepare(w) for w in books]
    w1 = [1.0] * len(books)
    merged = [s3_merge(r) for r in rows_s3]

    def old_path():
        m = [s3_merge(r) for r in rows_s3]
        for q, *_ in _hip.vq_forward_group(m, books, preps, False, w1):
            s3_split(q)

    arms = {"s3 filter": (1, lambda: _hip.vq_forward_group(rows_s3, books, preps, False, w1, s3=True)),
            "s3 exact (merge on load)": (0, lambda: _hip.vq_forward_group(rows_s3, books, preps, False, w1, s3=True)),
            "exact on merged rows": (1, lambda: _hip.vq_forward_group(merged, books, preps, False, w1)),
            "merge + exact + gather + split": (1, old_path)}
    res = {}
    for rep in range(reps):                                  # arms alternate
        for arm, (flt, fn) in arms.items():
            prev = _hip.set_option("vq_s3_filter", flt)
            res.setdefault(arm, []).append(timeit(fn, iters=10, warm=2))
            _hip.set_option("vq_s3_filter", prev)
    _hip.FILTER_DIAG = []
    _hip.vq_forward_group(rows_s3, books, preps, False, w1, s3=True)
    torch.cuda.synchronize()
    pairs = [(n, c, int(cnt[:64].sum()) / n) for n, c, _k, cnt in _hip.FILTER_DIAG]
    _hip.FILTER_DIAG = None
    print(f"[{name}] pairs per row: " + ", ".join(f"N{n}xC{c}: {p:.3f}" for n, c, p in pairs))
    for arm, v in res.items():
        v = sorted(v)
        print(f"[{name}] {arm:32s} median {v[len(v) // 2] * 1e3:7.1f} us   min {v[0] * 1e3:7.1f}  max {v[-1] * 1e3:7.1f}", flush=True)


def main_s3():
    from vq_seg_amd.vector_quantizer.vq_img import kmeans
    dev = torch.device("cuda:0")
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    K = 512
    print(torch.cuda.get_device_name(0), "B =", B, "K =", K)
    torch.manual_seed(0)
    rows, books = [], []
    for n, c in ((B * 4096, 512), (B * 1024, 1024), (B * 256, 2048)):      # post-ReLU features with channel-wise structure (vq_filter_bench.py)
        base = torch.relu(torch.randn(64, c, device=dev))
        mix = torch.softmax(2.0 * torch.randn(n, 64, device=dev), dim=1)
        x = s3_split(mix @ base + 0.1 * torch.relu(torch.randn(n, c, device=dev)))
        W, _ = kmeans(s3_merge(x), K, 10)
        rows.append(x)
        books.append(W.contiguous())
    s3_arm("k-means codebook", rows, books)
    del rows, books
    # the untrained network: codebooks k-means-initialised by its first training forward (as in the bench), rows = its eval features
    from tests import synth
    from vq_seg_amd import nnf
    from vq_seg_amd.models.networks import make_model
    from vq_seg_amd.utils.load_config import AttrDict
    model = make_model(AttrDict({"name": "vqreptunet1x1", "params": {
        "encoder_name": "resnet50", "num_classes": 3, "depth": 5,
        "vq_cfg": {"num_embeddings": [0, 0, K, K, K], "distance": "euclidean", "kmeans_init": True},
        "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}})).to(dev)
    x_l, _ = synth.blob_images(1, B, 512, cell=32)
    x_u, _ = synth.blob_images(2, B, 512, cell=32)
    with torch.no_grad():
        model.train()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            model.quantize(list(model.encode(x_l.to(dev))))           # k-means init of the three codebooks
        model.eval()
        feats = model.encode(x_u.to(dev))
    lv = [i for i in range(len(feats)) if isinstance(feats[i], nnf.S3) and hasattr(model.codebook[i], "codebook")]
    rows = [feats[i].rows.reshape(-1, 2 * feats[i].c) for i in lv]
    books = [model.codebook[i].codebook.embedding.weight.detach().contiguous() for i in lv]
    s3_arm("untrained network", rows, books)


if __name__ == "__main__":
    main_s3() if len(sys.argv) > 1 and sys.argv[1] == "s3" else main()
