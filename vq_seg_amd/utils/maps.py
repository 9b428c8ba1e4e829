"""What the integer-map utilities (utils.regions, utils.boundary) share: how a map comes in -- tensor or numpy array, with or without a
batch axis -- how a result goes back in the same form, and the shifted view of a map that their torch-op forms are built on."""
from __future__ import annotations

import numpy as np
import torch

INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def as_map(values, who):
    """(the (B, H, W) integer tensor, how to hand a result back: numpy or not, and whether a batch axis was added)"""
    is_np = isinstance(values, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(values)) if is_np else values
    if not torch.is_tensor(t) or t.dtype not in INT_DTYPES or t.dim() not in (2, 3):
        raise ValueError(f"{who}: an integer map (B, H, W) or (H, W) is required (uint8, int8, int16, int32 or int64), got "
                         f"{getattr(t, 'dtype', type(values).__name__)} {tuple(getattr(t, 'shape', ()))}")
    if t.numel() == 0:
        raise ValueError(f"{who}: an empty map, shape {tuple(t.shape)}")
    single = t.dim() == 2
    return (t[None] if single else t).detach(), is_np, single


def back(t, is_np, single):
    t = t[0] if single else t
    return t.cpu().numpy() if is_np else t


def shift(x, dy, dx, pad):
    """y[.., i, j] = x[.., i + dy, j + dx], `pad` where that is outside"""
    h, w = x.shape[-2:]
    out = torch.full_like(x, pad)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[..., yd, xd] = x[..., ys, xs]
    return out
