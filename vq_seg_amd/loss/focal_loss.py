"""Focal loss (reference: loss/focal_loss.py:6-68), same signatures and defaults.  Kept quirks: ignored pixels are not
skipped but become zero-logit class-0 pixels (:12-14), 'mean' divides by every pixel (:43), class weights normalise nothing
(:42 is overwritten by :43), and the MODULE softmaxes before it calls the function, which softmaxes again (:62-68).

One deviation, on the HIP path only: -log p_t is taken in log-softmax form.  Where a NON-target probability underflows to
exactly 0 the reference's `(-log p) * onehot` is inf * 0 = NaN; the kernel returns the finite value.  The two agree wherever
the reference is finite.  (The reference also stacks its ignore mask three times, :13, so it only runs for C = 3 -- and C = 1,
by broadcasting; here the mask is broadcast over any C.)"""
import torch
import torch.nn.functional as F
from torch import nn


def focal_supported(pred: torch.Tensor, num_classes: int, gamma) -> bool:
    """the HIP pass (vqseg_focal_*) takes 4-d float32 GPU logits with 2..4 classes and gamma == 0 or >= 1: between the two the
    derivative of (1 - p)^gamma is unbounded at p = 1, and that case stays on torch ops"""
    from .. import nnf
    return nnf.dice_sums_supported(pred, num_classes) and isinstance(gamma, (int, float)) and (gamma == 0 or gamma >= 1)


def _focal_torch(pred, target, alpha, gamma, num_classes, ignore_index, reduction, weight):
    """the reference's arithmetic, line by line (:9-50), with torch ops"""
    b, c = pred.shape[:2]
    pred = pred.reshape(b, c, -1)
    target = target.reshape(b, -1)
    mask = target != ignore_index if ignore_index is not None else torch.ones_like(target, dtype=torch.bool)
    pred = pred * mask.unsqueeze(1)                          # the reference stacks the mask 3x (:13)
    target = target * mask
    if num_classes == 1:
        pred = torch.sigmoid(pred)
    else:
        pred = F.softmax(pred, dim=1).float()
    onehot = torch.eye(num_classes, device=pred.device, dtype=pred.dtype)[target.long()].permute(0, 2, 1)
    if weight is not None:
        weight = weight[None, :, None].to(pred.device)
        onehot = onehot * weight
    focal = torch.pow(1 - pred, gamma)
    ce = -torch.log(pred)
    loss = torch.sum(alpha * focal * ce * onehot, dim=1)     # (B, HW)
    if reduction == "none":
        return loss
    if reduction == "mean":
        return torch.mean(loss)                              # every pixel; no division by sum(weight) (:42-43)
    if reduction == "sum":
        return torch.sum(loss)
    raise NotImplementedError(f"Invalid reduction mode: {reduction}")


def _focal(pred, target, alpha, gamma, num_classes, ignore_index, reduction, weight, pre_softmax):
    assert pred.shape[0] == target.shape[0], "pred tensor and target tensor must have same batch size"
    if focal_supported(pred, num_classes, gamma):
        from .. import nnf
        return nnf.focal(pred, target, alpha, gamma, ignore_index, reduction, weight, pre_softmax)     # HIP: one fused pass
    if pre_softmax:                                          # FocalLoss.forward (:63-66)
        pred = torch.sigmoid(pred) if num_classes == 1 else F.softmax(pred, dim=1).float()
    return _focal_torch(pred, target, alpha, gamma, num_classes, ignore_index, reduction, weight)


def focal_loss(pred: torch.Tensor, target: torch.Tensor, alpha, gamma, num_classes=3, ignore_index=None, reduction="sum",
               weight: torch.Tensor = None):
    return _focal(pred, target, alpha, gamma, num_classes, ignore_index, reduction, weight, False)


class FocalLoss(nn.Module):
    def __init__(self, num_classes, alpha=0.25, gamma=2, ignore_index=-100, reduction="mean", weight: torch.Tensor = None):
        super().__init__()
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.alpha = alpha
        self.gamma = gamma
        self.reduction = reduction
        self.weight = weight

    def forward(self, pred, target):
        return _focal(pred, target, self.alpha, self.gamma, self.num_classes, self.ignore_index, self.reduction, self.weight, True)
