"""RBD saliency maps over SLIC superpixels and salient masking (saliency_map/saliency.py:74-231, deprecated/train_salient.py:29-34).
The reference computes a map per image FILE on the host (skimage SLIC, Python loops over superpixel pairs, networkx all-pairs
shortest paths, a dense solve) and its trainers read the maps back from disk; here a whole batch is done on the device
(nnf.saliency_rbd: vqseg_slic_*_f, vqseg_region_graph_f, vqseg_rbd_*_f), on the images a training step actually forwards.

The definition is the one stated in include/vqseg.h: "Saliency Optimization from Robust Background Detection" (Zhu et al., CVPR 2014)
on this project's SLIC.  What differs from the reference: the superpixels are utils.superpixel's, not skimage's (no parity with the
reference's numbers is claimed); the map is in [0, 1] (the compat wrapper below multiplies by 255); there is no gray-image branch;
the degenerate divisions (a constant wCtr, a constant x) give 0; sigma_clr reaches the area sums (the reference's S() always uses 10).

Device tensors the kernels take go to them; CPU tensors, and whatever the kernels do not take, go through the torch-op form of the
same definition below (float32; float64 inputs stay float64).

    sal = saliency_rbd(images)                           # (B, H, W) float32 in [0, 1]
    masked = salient_masking(logits, sal, 0.1)           # differentiable in logits
"""
from __future__ import annotations

import numpy as np
import torch

from .. import nnf
from . import superpixel


# ---- the torch-op form, stage by stage (the same inputs and outputs as nnf._rbd_*) -----------------------------------------------
def _valid_labels(labels, grid):
    """labels (B, H, W) -> int64 with -1 where a label names no cluster of the 3 x 3 cells around the pixel's home cell"""
    gy, gx = grid
    b, h, w = labels.shape
    lv = labels.long()
    hi, hj = superpixel._home_cells(h, w, gy, gx, labels.device)
    ci, cj = lv.div(gx, rounding_mode="floor"), lv % gx
    ok = (lv >= 0) & (lv < gy * gx) & ((ci - hi[None, :, None]).abs() <= 1) & ((cj - hj[None, None, :]).abs() <= 1)
    return torch.where(ok, lv, torch.full_like(lv, -1))


def region_graph_torch(lab, labels, grid):
    """-> (stats (B, K, 8) = (L, a, b, y, x, n, bnd, 0) in lab's float type, adj uint8 (B, K, K))"""
    gy, gx = grid
    k = gy * gx
    b, _, h, w = lab.shape
    dev, dt = lab.device, lab.dtype
    lv = _valid_labels(labels, grid)
    ys = torch.arange(h, device=dev, dtype=dt)[:, None].expand(h, w)
    xs = torch.arange(w, device=dev, dtype=dt)[None, :].expand(h, w)
    edge = torch.zeros((h, w), dtype=dt, device=dev)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = 1, 1, 1, 1
    stats = torch.zeros((b, k, 8), dtype=dt, device=dev)
    adj = torch.zeros((b, k * k), dtype=torch.uint8, device=dev)
    for n in range(b):
        at = lv[n].reshape(-1)
        ok = at >= 0
        vals = torch.stack([lab[n, 0], lab[n, 1], lab[n, 2], ys, xs, torch.ones_like(ys), edge], dim=-1).reshape(-1, 7)
        sums = torch.zeros((k, 7), dtype=dt, device=dev).index_add_(0, at[ok], vals[ok])
        cnt = sums[:, 5]
        has = cnt > 0
        stats[n, has, :5] = sums[has, :5] / cnt[has][:, None]
        stats[n, :, 5] = cnt
        stats[n, :, 6] = (sums[:, 6] > 0).to(dt)
        for p, q in ((lv[n, :, :-1], lv[n, :, 1:]), (lv[n, :-1], lv[n, 1:])):
            p, q = p.reshape(-1), q.reshape(-1)
            e = (p >= 0) & (q >= 0) & (p != q)
            adj[n, p[e] * k + q[e]] = 1
            adj[n, q[e] * k + p[e]] = 1
    return stats, adj.reshape(b, k, k)


def weights_torch(stats, adj):
    act, bnd = stats[..., 5] > 0, stats[..., 6] > 0
    d = stats[:, :, None, :3] - stats[:, None, :, :3]
    dist = ((d[..., 0] ** 2 + d[..., 1] ** 2) + d[..., 2] ** 2).sqrt()
    edge = (adj.bool() | (bnd[:, :, None] & bnd[:, None, :])) & act[:, :, None] & act[:, None, :]
    wgt = torch.where(edge, dist, torch.full_like(dist, float("inf")))
    eye = torch.eye(stats.shape[1], dtype=torch.bool, device=stats.device)
    return torch.where(eye, torch.zeros_like(wgt), wgt)


def geodesic_torch(wgt):
    """Floyd-Warshall as K broadcast `minimum` steps"""
    g = wgt.clone()
    for k in range(g.shape[1]):
        g = torch.minimum(g, g[:, :, k:k + 1] + g[:, k:k + 1, :])
    return g


def background_torch(g, stats, sigma_clr=10.0, sigma_bndcon=1.0):
    act, bnd = stats[..., 5] > 0, stats[..., 6] > 0
    e = torch.where(act[:, None, :], torch.exp(-(g * g) / (2.0 * sigma_clr * sigma_clr)), torch.zeros_like(g))
    area = e.sum(-1)
    length = torch.where(bnd[:, None, :], e, torch.zeros_like(e)).sum(-1)
    bc = length / area.clamp_min(torch.finfo(g.dtype).tiny).sqrt()
    return torch.where(act, 1.0 - torch.exp(-(bc * bc) / (2.0 * sigma_bndcon * sigma_bndcon)), torch.zeros_like(bc))


def contrast_torch(g, stats, w_bg, h, w, sigma_spa=0.25):
    act = stats[..., 5] > 0
    dy, dx = stats[:, :, None, 3] - stats[:, None, :, 3], stats[:, :, None, 4] - stats[:, None, :, 4]
    d2 = (dy * dy + dx * dx) / float(h * h + w * w)
    both = act[:, :, None] & act[:, None, :]
    gf = torch.where(both, g, torch.zeros_like(g))           # +inf only where a cluster is inactive: never multiplied
    return (gf * torch.exp(-d2 / (2.0 * sigma_spa * sigma_spa)) * w_bg[:, None, :]).sum(-1)


def _unit_range(v, act):
    """(v - min) / (max - min) over the active clusters, per image; 0 where inactive or where max = min"""
    inf = torch.full_like(v, float("inf"))
    lo, hi = torch.where(act, v, inf).amin(-1, keepdim=True), torch.where(act, v, -inf).amax(-1, keepdim=True)
    ok = act & (hi > lo)
    span = torch.where(hi > lo, hi - lo, torch.ones_like(hi))
    return torch.where(ok, (torch.where(act, v, lo.expand_as(v)) - lo) / span, torch.zeros_like(v))


def solve_torch(g, stats, adj, w_bg, wctr, sigma_clr=10.0, mu=0.1):
    """-> (wCtr normalised, x, x normalised)"""
    act = stats[..., 5] > 0
    both = act[:, :, None] & act[:, None, :]
    wn = _unit_range(wctr, act)
    s = torch.where(adj.bool() & both, torch.exp(-(g * g) / (2.0 * sigma_clr * sigma_clr)) + mu, torch.zeros_like(g))
    diag = torch.where(act, (2.0 * w_bg + 2.0 * wn) + 2.0 * s.sum(-1), torch.ones_like(wn))
    a = torch.diag_embed(diag) - 2.0 * s
    x = torch.linalg.solve(a, (2.0 * wn).unsqueeze(-1)).squeeze(-1)
    x = torch.where(act, x, torch.zeros_like(x))
    return wn, x, _unit_range(x, act)


def paint_torch(xnorm, labels, grid):
    lv = _valid_labels(labels, grid)
    b, h, w = lv.shape
    sal = torch.gather(xnorm, 1, lv.clamp_min(0).reshape(b, -1)).reshape(b, h, w)
    return torch.where(lv >= 0, sal, torch.zeros_like(sal))


def _check_from_labels(lab, labels, grid):
    if not (torch.is_tensor(lab) and torch.is_tensor(labels) and lab.dim() == 4 and lab.shape[1] == 3 and labels.dim() == 3
            and labels.shape[0] == lab.shape[0] and labels.shape[1:] == lab.shape[2:]):
        raise ValueError(f"saliency_rbd_from_labels: lab (B, 3, H, W) and labels (B, H, W) of one batch and size, got "
                         f"{tuple(getattr(lab, 'shape', ()))} and {tuple(getattr(labels, 'shape', ()))}")
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"saliency_rbd_from_labels: labels must be an integer tensor, got {labels.dtype}")
    gy, gx = int(grid[0]), int(grid[1])
    if not (1 <= gy <= lab.shape[2] and 1 <= gx <= lab.shape[3]):
        raise ValueError(f"saliency_rbd_from_labels: the grid must have 1..H rows and 1..W columns of cells, got {grid!r}")
    return gy, gx


def saliency_rbd_from_labels_torch(lab, labels, grid, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1, return_parts=False):
    """the torch-op form of nnf.rbd_from_labels on any device; float32 unless `lab` is float64"""
    gy, gx = _check_from_labels(lab, labels, grid)
    sigma_clr, sigma_bndcon, sigma_spa, mu = nnf.rbd_settings(sigma_clr, sigma_bndcon, sigma_spa, mu)
    lab = lab.detach()
    lab = lab if lab.dtype == torch.float64 else lab.float()
    labels = labels.detach().to(lab.device)
    h, w = lab.shape[2:]
    stats, adj = region_graph_torch(lab, labels, (gy, gx))
    g = geodesic_torch(weights_torch(stats, adj))
    w_bg = background_torch(g, stats, sigma_clr, sigma_bndcon)
    wctr = contrast_torch(g, stats, w_bg, h, w, sigma_spa)
    wn, x, xnorm = solve_torch(g, stats, adj, w_bg, wctr, sigma_clr, mu)
    sal = paint_torch(xnorm, labels, (gy, gx))
    if return_parts:
        return sal, dict(stats=stats, adj=adj, geodesic=g, w_bg=w_bg, wctr=wctr, wctr_norm=wn, x=x, xnorm=xnorm)
    return sal


def _kernels_take(lab, labels, grid):
    return (torch.is_tensor(lab) and torch.is_tensor(labels) and lab.is_cuda and labels.device == lab.device and lab.dtype == torch.float32
            and labels.dtype == torch.int32 and lab.dim() == 4 and labels.dim() == 3 and 1 <= lab.shape[0] <= 65535
            and max(lab.shape[2:]) <= nnf.SLIC_MAX_SIDE and int(grid[0]) * int(grid[1]) <= nnf.RBD_MAX_SEGMENTS)


def saliency_rbd_from_labels(lab, labels, grid, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1, return_parts=False):
    """RBD saliency of planar Lab images (B, 3, H, W) under a SLIC label map (B, H, W) of the grid (gy, gx) -> (B, H, W) in [0, 1].
    Only label maps as slic makes them: a label outside the 3 x 3 cells around its pixel's home cell is ignored.  The kernels for
    float32 / int32 GPU tensors with at most nnf.RBD_MAX_SEGMENTS cells, else the torch-op form."""
    _check_from_labels(lab, labels, grid)
    if _kernels_take(lab, labels, grid):
        return nnf.rbd_from_labels(lab, labels, grid, sigma_clr, sigma_bndcon, sigma_spa, mu, return_parts)
    return saliency_rbd_from_labels_torch(lab, labels, grid, sigma_clr, sigma_bndcon, sigma_spa, mu, return_parts)


def saliency_rbd_from_slic(images, labels, grid, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1):
    """saliency_rbd of `images` (B, 3, H, W) under label maps that slic already made of them (`labels`, `grid` as slic returns them):
    only the Lab conversion is repeated, so the map equals saliency_rbd(images, ...) with the same SLIC settings bit for bit"""
    gy, gx = int(grid[0]), int(grid[1])
    if nnf.slic_supported(images) and _kernels_take(images, labels, grid):
        lab = nnf._slic_lab(images.detach(), gy, gx)[0]
    else:
        images = images.detach()
        lab = superpixel.rgb_to_lab(images if images.dtype == torch.float64 else images.float())
    return saliency_rbd_from_labels(lab, labels, (gy, gx), sigma_clr, sigma_bndcon, sigma_spa, mu)


def saliency_rbd_torch(images, n_segments=250, compactness=10.0, iters=10, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1,
                       return_parts=False):
    """the torch-op form of nnf.saliency_rbd on any device: slic_torch, then saliency_rbd_from_labels_torch"""
    labels, _centers, grid = superpixel.slic_torch(images, n_segments, compactness, iters)
    images = images.detach()
    lab = superpixel.rgb_to_lab(images if images.dtype == torch.float64 else images.float())
    return saliency_rbd_from_labels_torch(lab, labels, grid, sigma_clr, sigma_bndcon, sigma_spa, mu, return_parts)


def saliency_rbd(images, n_segments=250, compactness=10.0, iters=10, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1,
                 return_parts=False):
    """RBD saliency maps of `images` (B, 3, H, W) in [0, 1] -> (B, H, W) in [0, 1], one per image; 250 superpixels and the sigmas are
    the reference's values (saliency.py:74-80).  The kernels where nnf.rbd_supported, else the torch-op form.  No gradient flows."""
    if not (torch.is_tensor(images) and images.dim() == 4 and images.shape[1] == 3):
        raise ValueError(f"saliency_rbd: images must be a (B, 3, H, W) tensor, got {tuple(getattr(images, 'shape', ()))}")
    if nnf.rbd_supported(images, n_segments):
        return nnf.saliency_rbd(images.detach(), n_segments, compactness, iters, sigma_clr, sigma_bndcon, sigma_spa, mu, return_parts)
    return saliency_rbd_torch(images, n_segments, compactness, iters, sigma_clr, sigma_bndcon, sigma_spa, mu, return_parts)


def salient_masking(pred, saliency, threshold=0.1):
    """train_salient.py:29-34: the scores of every class >= 1 are multiplied by 0 where saliency <= threshold; class 0 is untouched.
    pred (B, C, H, W) of any float type, saliency (B, H, W); differentiable in `pred`."""
    if not (torch.is_tensor(pred) and torch.is_tensor(saliency) and pred.dim() == 4 and saliency.dim() == 3
            and saliency.shape[0] == pred.shape[0] and saliency.shape[1:] == pred.shape[2:]):
        raise ValueError(f"salient_masking: pred (B, C, H, W) and saliency (B, H, W) of one batch and size, got "
                         f"{tuple(getattr(pred, 'shape', ()))} and {tuple(getattr(saliency, 'shape', ()))}")
    if not pred.dtype.is_floating_point:
        raise ValueError(f"salient_masking: pred must be a float tensor, got {pred.dtype}")
    keep = (saliency.detach() > threshold).to(pred.dtype).unsqueeze(1)                    # (B, 1, H, W): 0 on the background
    first = torch.zeros((1, pred.shape[1], 1, 1), dtype=torch.bool, device=pred.device)
    first[:, 0] = True
    return pred * torch.where(first, torch.ones_like(keep), keep)


# ---- the reference's entry points (compat/saliency_map) --------------------------------------------------------------------------
def get_saliency_rbd(img_path_or_array, n_segments=250, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1, resize=(512, 512)):
    """saliency.py:74-231's call: an image file (opened with PIL, resized bilinear to `resize` unless it is None) or a numpy array
    (H, W, 3) or (H, W), taken as is (uint8 0..255 or float 0..1) -> float64 numpy (H, W) in 0..255.  On the GPU when there is one."""
    if isinstance(img_path_or_array, np.ndarray):
        arr = img_path_or_array
    else:
        from PIL import Image
        with Image.open(img_path_or_array) as im:
            im = im.convert("RGB")
            if resize:
                im = im.resize((int(resize[1]), int(resize[0])), Image.BILINEAR)
            arr = np.asarray(im)
    if arr.ndim == 2:
        arr = np.stack([arr] * 3, axis=-1)
    if arr.ndim != 3 or arr.shape[2] != 3:
        raise ValueError(f"get_saliency_rbd: an image of shape (H, W, 3) or (H, W), got {arr.shape}")
    scale = 255.0 if arr.dtype == np.uint8 else 1.0
    img = torch.from_numpy(np.ascontiguousarray(arr).astype(np.float32) / scale).permute(2, 0, 1)[None].contiguous()
    if torch.cuda.is_available():
        img = img.cuda()
    sal = saliency_rbd(img, n_segments, sigma_clr=sigma_clr, sigma_bndcon=sigma_bndcon, sigma_spa=sigma_spa, mu=mu)
    return 255.0 * sal[0].double().cpu().numpy()


def get_saliency_ft(img_path):
    raise NotImplementedError("get_saliency_ft (frequency-tuned saliency, saliency.py:233) is not built: only get_saliency_rbd is")
