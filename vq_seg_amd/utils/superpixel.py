"""SLIC superpixels and superpixel-mean pooling (deprecated/train_slic.py:44-69,152-160; deprecated/obia_pseudolabel.py and
saliency_map/saliency.py sit on the same primitive).  The reference calls fast_slic on the host, four times per training step; here
the label maps are made on the device (nnf.slic: vqseg_slic_lab_f / _assign_f / _update_f) and the pooling is two launches
(nnf.segment_mean: vqseg_segment_sums_f / _broadcast_f) with a backward pass that is the same two.

The algorithm is the one stated in include/vqseg.h -- SLIC in its gather (gSLIC) form on float CIELAB, a regular gy x gx grid, a
3 x 3 candidate window around the home cell, no connectivity enforcement (utils.regions.enforce_connectivity is a pass of its own) -- NOT fast_slic's: that library quantises the image to
uint8, and neither it nor skimage is available to compare against, so no parity with either is claimed.  The pooling is the mean of
the class scores over each superpixel, which train_slic.py:62-69 evidently means (as written it reduces over the wrong axes and
multiplies the prediction by means / prediction).

Device tensors the kernels take go to them; CPU tensors, and whatever the kernels do not take, go through the torch-op form of the
same definition below (float32, index_add_ for the sums; float64 inputs stay float64).

    labels = slic(images, 1600)                          # (B, H, W) int32
    pooled = superpixel_mean(logits, labels)             # differentiable in logits
"""
from __future__ import annotations

import torch

from .. import nnf


def superpixel_grid(h: int, w: int, num_components: int):
    """(gy, gx): S = sqrt(h w / K), gy = max(1, round(h / S)), gx = max(1, round(w / S)); K_eff = gy * gx superpixels, indexed i * gx + j"""
    return nnf.slic_grid(h, w, num_components)


def rgb_to_lab(images: torch.Tensor) -> torch.Tensor:
    """(B, 3, H, W) sRGB in [0, 1] -> CIELAB with torch ops, in the images' float type (the formulas of include/vqseg.h)"""
    lin = torch.where(images > 0.04045, ((images.clamp_min(0.0) + 0.055) / 1.055) ** 2.4, images / 12.92)
    r, g, b = lin[:, 0], lin[:, 1], lin[:, 2]
    x = (r * 0.412453 + g * 0.357580 + b * 0.180423) / 0.95047
    y = r * 0.212671 + g * 0.715160 + b * 0.072169
    z = (r * 0.019334 + g * 0.119193 + b * 0.950227) / 1.08883

    def f(t):
        return torch.where(t > 0.008856, torch.sign(t) * t.abs() ** (1.0 / 3.0), 7.787 * t + 16.0 / 116.0)
    fx, fy, fz = f(x), f(y), f(z)
    return torch.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], dim=1)


def _home_cells(h, w, gy, gx, dev):
    return (torch.arange(h, device=dev) * gy).div(h, rounding_mode="floor"), (torch.arange(w, device=dev) * gx).div(w, rounding_mode="floor")


def _assign_torch(lab, centers, gy, gx, weight):
    """labels (B, H, W) int64: the nearest of the clusters of the 3 x 3 cells around the home cell, ties to the lowest index"""
    b, _, h, w = lab.shape
    dev = lab.device
    hi, hj = _home_cells(h, w, gy, gx, dev)
    ys = torch.arange(h, device=dev, dtype=lab.dtype)[:, None]
    xs = torch.arange(w, device=dev, dtype=lab.dtype)[None, :]
    best = torch.full((b, h, w), float("inf"), dtype=lab.dtype, device=dev)
    label = (hi[:, None] * gx + hj[None, :]).expand(b, h, w).clone()
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ci, cj = hi + di, hj + dj
            ok = ((ci >= 0) & (ci < gy))[:, None] & ((cj >= 0) & (cj < gx))[None, :]
            idx = ci.clamp(0, gy - 1)[:, None] * gx + cj.clamp(0, gx - 1)[None, :]              # (H, W)
            c = centers[:, idx]                                                                   # (B, H, W, 5)
            d = ((lab[:, 0] - c[..., 0]) ** 2 + (lab[:, 1] - c[..., 1]) ** 2 + (lab[:, 2] - c[..., 2]) ** 2) \
                + weight * ((ys - c[..., 3]) ** 2 + (xs - c[..., 4]) ** 2)
            win = ok & (d < best)
            best = torch.where(win, d, best)
            label = torch.where(win, idx, label)
    return label


def _update_torch(lab, labels, centers):
    """the mean of (L, a, b, y, x) over each cluster's pixels (index_add_); a cluster without pixels keeps its centre"""
    b, _, h, w = lab.shape
    k = centers.shape[1]
    dev = lab.device
    ys = torch.arange(h, device=dev, dtype=lab.dtype)[:, None].expand(h, w)
    xs = torch.arange(w, device=dev, dtype=lab.dtype)[None, :].expand(h, w)
    out = centers.clone()
    for n in range(b):
        vals = torch.stack([lab[n, 0], lab[n, 1], lab[n, 2], ys, xs], dim=-1).reshape(-1, 5)
        at = labels[n].reshape(-1)
        sums = torch.zeros((k, 5), dtype=lab.dtype, device=dev).index_add_(0, at, vals)
        cnt = torch.zeros(k, dtype=lab.dtype, device=dev).index_add_(0, at, torch.ones_like(vals[:, 0]))
        has = cnt > 0
        out[n, has] = sums[has] / cnt[has][:, None]
    return out


def slic_torch(images: torch.Tensor, num_components: int, compactness: float = 10.0, iters: int = 10):
    """the torch-op form of nnf.slic on any device: (labels int32 (B, H, W), centers (B, K_eff, 5), (gy, gx)); float32 unless the
    images are float64"""
    if not (torch.is_tensor(images) and images.dim() == 4 and images.shape[1] == 3):
        raise ValueError(f"slic: images must be a (B, 3, H, W) tensor, got {tuple(getattr(images, 'shape', ()))}")
    b, _, h, w = images.shape
    gy, gx, weight, iters = nnf.slic_settings(h, w, num_components, compactness, iters)
    images = images.detach()
    images = images if images.dtype == torch.float64 else images.float()
    lab = rgb_to_lab(images)
    sy = torch.tensor([((2 * i + 1) * h) // (2 * gy) for i in range(gy)], device=images.device)
    sx = torch.tensor([((2 * j + 1) * w) // (2 * gx) for j in range(gx)], device=images.device)
    yy, xx = sy[:, None].expand(gy, gx).reshape(-1), sx[None, :].expand(gy, gx).reshape(-1)
    centers = torch.cat([lab[:, :, yy, xx].permute(0, 2, 1), yy.to(lab.dtype).expand(b, -1)[..., None], xx.to(lab.dtype).expand(b, -1)[..., None]], dim=2)
    for _ in range(iters):
        centers = _update_torch(lab, _assign_torch(lab, centers, gy, gx, weight), centers)
    return _assign_torch(lab, centers, gy, gx, weight).to(torch.int32), centers, (gy, gx)


def slic(images: torch.Tensor, num_components: int = 1600, compactness: float = 10.0, iters: int = 10, return_centers: bool = False):
    """SLIC superpixels of `images` (B, 3, H, W) in [0, 1] -> labels int32 (B, H, W) in [0, K_eff), K_eff = gy * gx of
    superpixel_grid; with `return_centers` -> (labels, centers float (B, K_eff, 5) = (L, a, b, y, x), (gy, gx)).  `num_components`
    1600 is the reference's value (train_slic.py:49).  The kernels where nnf.slic_supported, else the torch-op form."""
    out = nnf.slic(images.detach(), num_components, compactness, iters) if nnf.slic_supported(images) else \
        slic_torch(images, num_components, compactness, iters)
    return out if return_centers else out[0]


class _SegmentMeanTorch(torch.autograd.Function):
    """the torch-op form of nnf.segment_mean (index_add_ for the sums), in x's float type; its backward is itself"""

    @staticmethod
    def forward(ctx, x, labels, k):
        ctx.save_for_backward(labels)
        ctx.k = k
        return _SegmentMeanTorch.pool(x, labels, k)

    @staticmethod
    def pool(x, labels, k):
        b, c, h, w = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(b, h * w, c)
        out = rows.clone()
        for n in range(b):
            at = labels[n].reshape(-1).long()
            ok = (at >= 0) & (at < k)
            idx = at[ok]
            sums = torch.zeros((k, c), dtype=x.dtype, device=x.device).index_add_(0, idx, rows[n][ok])
            cnt = torch.zeros(k, dtype=x.dtype, device=x.device).index_add_(0, idx, torch.ones(idx.shape[0], dtype=x.dtype, device=x.device))
            out[n][ok] = sums[idx] / cnt[idx][:, None]
        return out.reshape(b, h, w, c).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        (labels,) = ctx.saved_tensors
        return _SegmentMeanTorch.pool(g, labels, ctx.k), None, None


def superpixel_mean(pred: torch.Tensor, labels: torch.Tensor, num_segments=None) -> torch.Tensor:
    """pred (B, C, H, W) averaged over the segments of `labels` (B, H, W), per image: every pixel gets the mean of its segment, for
    any label map; a label outside [0, num_segments) leaves its pixel as it is.  `num_segments` None: labels.max() + 1 (a host
    read; give it where that matters).  Differentiable in `pred`; the backward pass is the same pooling of the incoming gradient."""
    if not (torch.is_tensor(pred) and torch.is_tensor(labels) and pred.dim() == 4 and labels.dim() == 3
            and labels.shape[0] == pred.shape[0] and labels.shape[1:] == pred.shape[2:]):
        raise ValueError(f"superpixel_mean: pred (B, C, H, W) and labels (B, H, W) of one batch and size, got "
                         f"{tuple(getattr(pred, 'shape', ()))} and {tuple(getattr(labels, 'shape', ()))}")
    if labels.dtype.is_floating_point or labels.dtype in (torch.bool,):
        raise ValueError(f"superpixel_mean: labels must be an integer tensor, got {labels.dtype}")
    k = int(labels.max()) + 1 if num_segments is None else int(num_segments)
    if k < 1:
        raise ValueError(f"superpixel_mean: num_segments must be positive, got {k}")
    if nnf.segment_mean_supported(pred, labels):
        return nnf.segment_mean(pred, labels, k)
    if not pred.dtype.is_floating_point:
        raise ValueError(f"superpixel_mean: pred must be a float tensor, got {pred.dtype}")
    x = pred if pred.dtype in (torch.float32, torch.float64) else pred.float()
    return _SegmentMeanTorch.apply(x, labels.detach().to(x.device), k)
