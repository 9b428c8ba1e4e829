"""Dense-CRF refinement of a prediction (reference: utils/crf.py `DenseCRF`, run by deprecated/test _crf.py after the forward and
before the metrics).

The reference wraps pydensecrf, a CPU library that filters through a permutohedral lattice.  Here the same model -- Krähenbühl &
Koltun's mean-field inference with a Potts compatibility, a positional and a bilateral Gaussian kernel and symmetric kernel
normalisation, the wrapped library's defaults -- is computed EXACTLY over all pixel pairs of a truncated support (the contract of
include/vqseg.h, restated in float64 in tests/crf_cases.py):

    rgb = trunc(clamp(image, 0, 1) * 255),  U = -log(clip(prob, 1e-5, 1)),  Q0 = softmax(-U)
    k_pos = exp(-|dp|^2 / (2 pos_xy_std^2)),  k_bi = exp(-|dp|^2 / (2 bi_xy_std^2) - |drgb|^2 / (2 bi_rgb_std^2)),  j = i included,
    k = 0 unless |dx|, |dy| <= R = ceil(truncate * xy_std) of that kernel (truncate None: everywhere)
    n_i = 1 / sqrt(sum_j k(i, j) + 1e-20),  m_i = n_i sum_j k(i, j) n_j Q_j,  Q_i = softmax(-U_i + pos_w m_pos,i + bi_w m_bi,i)

No parity with the lattice approximation is claimed.  Device tensors take the HIP kernels (nnf.dense_crf); numpy arrays and CPU
tensors take the torch-op form below, which works in chunks of rows and in float64 (the convention of utils/visualize.py).

    DenseCRF()(image, prob_map)                   # the reference's call: (3, H, W), (C, H, W) -> (C, H, W)
    DenseCRF(truncate=None).batch(images, probs, out="logits")
"""
import math

import torch

from .. import nnf

_CHUNK_ELEMS = 1 << 22            # elements of one (rows of i) x (window of j) block of the torch-op form
_CACHE_ELEMS = 1 << 24            # all blocks together up to this many elements: built once, not once per iteration


def _radius(truncate, xy_std, h, w):
    far = max(h, w) - 1
    r = math.ceil(truncate * xy_std) if math.isfinite(truncate * xy_std) else far
    return min(r, far)


def _blocks(h, w, rb, rp):
    """the row chunks of the torch-op form: (i rows r0..r1, j rows s0..s1) with every j row some i row can see"""
    rw = max(rb, rp)
    rows = max(1, min(h, _CHUNK_ELEMS // max(1, w * w * min(h, 2 * rw + 8))))
    for r0 in range(0, h, rows):
        r1 = min(h, r0 + rows)
        yield r0, r1, max(0, r0 - rw), min(h, r1 + rw)


def mean_field_torch(image, prob, iter_max=10, bi_w=7.0, bi_xy_std=50.0, bi_rgb_std=4.0, pos_w=3.0, pos_xy_std=3.0, truncate=4.0,
                     dtype=torch.float64, keep=None):
    """The contract with torch ops for ONE image: image (3, H, W) in [0, 1], prob (C, H, W) -> (Q (C, H, W), E (C, H, W)) in `dtype`
    on the inputs' device, E the last update's energies (iter_max = 0: -U).  The kernel blocks are built in chunks of rows (per iteration
    once an image is too large to hold them), so nothing of size (H W)^2 is held for a large image.  `keep`: a dict that receives {iteration: Q} after every update (tests measure
    float32 against float64 through it)."""
    iters, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, trunc = nnf.crf_settings(iter_max, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std,
                                                                                  truncate, who="DenseCRF")
    c, h, w = prob.shape
    dev = prob.device
    rgb = (image.detach().to(torch.float32).clamp(0.0, 1.0) * 255.0).to(torch.uint8).to(dtype).reshape(3, h * w).t()      # (N, 3) integers
    u = -torch.log(prob.detach().to(dtype).clamp(1e-5, 1.0)).reshape(c, h * w).t()                                        # (N, C)
    q = torch.softmax(-u, dim=1)
    e = -u
    if iters == 0:
        return q.t().reshape(c, h, w), e.t().reshape(c, h, w)
    rb, rp = _radius(trunc, bi_xy_std, h, w), _radius(trunc, pos_xy_std, h, w)
    ys, xs = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
    ys, xs = ys.reshape(-1), xs.reshape(-1)

    def kernels(r0, r1, s0, s1):
        i, j = slice(r0 * w, r1 * w), slice(s0 * w, s1 * w)
        dx, dy = (xs[i, None] - xs[None, j]), (ys[i, None] - ys[None, j])
        d2 = (dx * dx + dy * dy).to(dtype)
        c2 = sum((rgb[i, None, ch] - rgb[None, j, ch]) ** 2 for ch in range(3))
        adx, ady = dx.abs(), dy.abs()
        kb = torch.exp(-0.5 * (d2 / bi_xy_std ** 2 + c2 / bi_rgb_std ** 2)) * ((adx <= rb) & (ady <= rb))
        kp = torch.exp(-0.5 * d2 / pos_xy_std ** 2) * ((adx <= rp) & (ady <= rp))
        return i, j, kb, kp

    nb, np_ = torch.empty(h * w, dtype=dtype, device=dev), torch.empty(h * w, dtype=dtype, device=dev)
    blocks = list(_blocks(h, w, rb, rp))
    held = sum((r1 - r0) * (s1 - s0) * w * w for r0, r1, s0, s1 in blocks)
    cache = [kernels(*blk) for blk in blocks] if held <= _CACHE_ELEMS else None       # a small image: its blocks are built once
    for n, blk in enumerate(blocks):
        i, j, kb, kp = cache[n] if cache else kernels(*blk)
        nb[i], np_[i] = 1.0 / torch.sqrt(kb.sum(dim=1) + 1e-20), 1.0 / torch.sqrt(kp.sum(dim=1) + 1e-20)
    for it in range(iters):
        e = torch.empty_like(u)
        for n, blk in enumerate(blocks):
            i, j, kb, kp = cache[n] if cache else kernels(*blk)
            mb = nb[i, None] * (kb @ (nb[j, None] * q[j]))
            mp = np_[i, None] * (kp @ (np_[j, None] * q[j]))
            e[i] = -u[i] + pos_w * mp + bi_w * mb
        q = torch.softmax(e, dim=1)
        if keep is not None:
            keep[it + 1] = q.t().reshape(c, h, w)
    return q.t().reshape(c, h, w), e.t().reshape(c, h, w)


class DenseCRF:
    """The reference's constructor order (utils/crf.py:6) plus `truncate`: the support of both kernels is |dx|, |dy| <=
    ceil(truncate * xy_std); None: every pixel pair."""

    def __init__(self, iter_max=10, bi_w=7, bi_xy_std=50, bi_rgb_std=4, pos_w=3, pos_xy_std=3, truncate=4.0):
        nnf.crf_settings(iter_max, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, truncate, who="DenseCRF")
        self.iter_max, self.bi_w, self.bi_xy_std, self.bi_rgb_std = iter_max, bi_w, bi_xy_std, bi_rgb_std
        self.pos_w, self.pos_xy_std, self.truncate = pos_w, pos_xy_std, truncate

    def settings(self):
        return dict(iter_max=self.iter_max, bi_w=self.bi_w, bi_xy_std=self.bi_xy_std, bi_rgb_std=self.bi_rgb_std, pos_w=self.pos_w,
                    pos_xy_std=self.pos_xy_std, truncate=self.truncate)

    def __call__(self, image, prob_map):
        """image (3, H, W) in [0, 1], prob_map (C, H, W) -> Q (C, H, W): a float32 numpy array for numpy arrays and CPU tensors (as
        the reference returns), a device tensor for device tensors (the HIP kernels)."""
        image, prob_map = torch.as_tensor(image), torch.as_tensor(prob_map)
        if image.dim() != 3 or prob_map.dim() != 3 or image.shape[0] != 3 or tuple(image.shape[1:]) != tuple(prob_map.shape[1:]):
            raise ValueError(f"DenseCRF: image (3, H, W) and prob_map (C, H, W) of one size expected, got {tuple(image.shape)} and "
                             f"{tuple(prob_map.shape)}")
        if prob_map.shape[0] < 2:
            raise ValueError(f"DenseCRF: at least 2 classes, got {prob_map.shape[0]}")
        if prob_map.is_cuda:
            return self.batch(image.to(prob_map.device)[None], prob_map[None])[0]
        q, _ = mean_field_torch(image.cpu(), prob_map, **self.settings())
        return q.to(torch.float32).numpy()

    @torch.no_grad()
    def batch(self, images, probs, out="prob"):
        """images (B, 3, H, W), probs (B, C, H, W) -> Q or, with out="logits", the last energies (B, C, H, W) float32 on the inputs'
        device: nnf.dense_crf on the GPU, the torch-op form image by image elsewhere."""
        if out not in ("prob", "logits"):
            raise ValueError(f"DenseCRF.batch: out is 'prob' or 'logits', got {out!r}")
        if probs.is_cuda:
            return nnf.dense_crf(images.float(), probs.float(), out=out, **self.settings())
        if images.dim() != 4 or probs.dim() != 4 or images.shape[0] != probs.shape[0]:
            raise ValueError(f"DenseCRF.batch: images (B, 3, H, W) and probs (B, C, H, W) expected, got {tuple(images.shape)} and {tuple(probs.shape)}")
        res = [mean_field_torch(i, p, **self.settings())[out == "logits"] for i, p in zip(images, probs)]
        return torch.stack(res).to(torch.float32)
