"""Loss factory (reference: loss/__init__.py:5-33): make_loss, make_loss_as_func, compute_class_weight.  dice + cross-entropy are
the ones the default path uses; the class-balanced and focal criteria ride the same fused passes (nnf.focal, nnf.wce_sums)."""
import torch
import torch.nn.functional as F
from torch import nn

from .dice_loss import DiceLoss, dice_loss  # noqa: F401
from .focal_loss import FocalLoss, focal_loss  # noqa: F401
from .contrastive_loss import SupConLoss  # noqa: F401  (not a criterion of the factory: loss_dict keeps the reference's four keys)
from .conf_ce_loss import ConfCELoss, conf_ce_loss, unreliable_weight  # noqa: F401  (not in loss_func_dict: its entries take labels)


def cross_entropy(input, target, weight=None, *args, **kwargs):
    """F.cross_entropy; with class weights that live on the GPU and (B, C, H, W) float32 logits of 2..4 classes the weighted mean
    comes from one pass over the logits (nnf.wce_sums) and the weights stay on the device -- the per-step weights of
    compute_class_weight (deprecated/train_vq_pt_unet_balncedweightedloss.py:135-141).  Anything else is F.cross_entropy."""
    from .. import nnf
    plain = not args and set(kwargs) <= {"ignore_index", "reduction"} and kwargs.get("reduction", "mean") == "mean"
    if plain and torch.is_tensor(weight) and weight.is_cuda and nnf.dice_sums_supported(input, input.shape[1]) and \
            not target.is_floating_point() and target.dim() == 3:
        ce = nnf.wce_sums(input, target, weight, kwargs.get("ignore_index", -100))
        return ce[:, 0].sum() / ce[:, 1].sum()
    return F.cross_entropy(input, target, weight, *args, **kwargs)


loss_dict = {"cross_entropy": nn.CrossEntropyLoss, "dice_loss": DiceLoss, "focal_loss": FocalLoss, "nll_loss": nn.NLLLoss}

loss_func_dict = {"cross_entropy": cross_entropy, "dice_loss": dice_loss, "focal_loss": focal_loss, "nll_loss": F.nll_loss}


def make_loss(loss_name: str, num_classes: int, ignore_index: int = -100, weight=None):
    if loss_name in ("cross_entropy", "nll_loss"):
        return loss_dict[loss_name](ignore_index=ignore_index, weight=weight)
    if loss_name not in loss_dict:
        raise KeyError(f"loss {loss_name!r} is not on the accelerated path; available: {sorted(loss_dict)}")
    return loss_dict[loss_name](num_classes=num_classes, ignore_index=ignore_index, weight=weight)


def make_loss_as_func(loss_name: str):
    return loss_func_dict[loss_name]


def compute_class_weight(num_classes, y: torch.Tensor):
    """1 - (share of each class among the labels) (:28-33).  Labels on the GPU: one counting pass (nnf.class_weight) instead of
    torch.bincount, which waits for the device to size its output; the weights are made and stay on the device.  One difference:
    a label >= num_classes (an ignore value such as 255) makes bincount's vector, and so the reference's result, longer than
    num_classes; here such labels count in the total, as there, but the result always has num_classes entries."""
    if y.is_cuda:
        from .. import nnf
        return nnf.class_weight(num_classes, y)[0]
    class_sample_count = torch.bincount(torch.flatten(y), minlength=num_classes)
    class_sample_prob = class_sample_count / torch.sum(class_sample_count)
    return 1. - class_sample_prob
