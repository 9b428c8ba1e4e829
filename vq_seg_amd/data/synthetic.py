"""Synthetic data (no dataset is available offline; shapes and value ranges of data/dataset.py:41-62)."""
import torch
import torch.nn.functional as F

from .. import dist as vdist


class SyntheticCropWeed:
    """Images: learnable colour-coded blobs + noise in [0,1] (TF.to_tensor range, no mean/std
    normalisation, q14); labels: class ids 0/1/2 (post `img_to_label`).  Deterministic per (seed, rank)."""

    def __init__(self, size: int, batch: int, device, seed: int = 42, cell: int = 32, num_classes: int = 3):
        self.size, self.batch, self.device, self.cell, self.nc = size, batch, device, cell, num_classes
        self.gen = torch.Generator(device="cpu")
        self.gen.manual_seed(seed * 1000 + vdist.rank())
        self.palette = torch.tensor([[0.25, 0.20, 0.15], [0.20, 0.55, 0.25], [0.55, 0.60, 0.20]])

    def _one(self):
        low = max(self.size // self.cell, 1)
        lab = torch.randint(0, self.nc, (self.batch, 1, low, low), generator=self.gen).float()
        lab = F.interpolate(lab, size=(self.size, self.size), mode="nearest")[:, 0].long()
        img = self.palette[lab].permute(0, 3, 1, 2) + 0.15 * torch.rand(self.batch, 3, self.size, self.size, generator=self.gen)
        return img.clamp_(0, 1), lab

    def labelled(self):
        img, lab = self._one()
        return img.to(self.device, non_blocking=True), lab.to(self.device, non_blocking=True)

    def unlabelled(self):
        return self._one()[0].to(self.device, non_blocking=True)
