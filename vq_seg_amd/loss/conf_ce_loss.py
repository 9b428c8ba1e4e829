"""Confidence-weighted soft cross-pseudo-supervision loss (reference: conf_ce_loss and cal_unsuploss_weight of
deprecated/train_vq_pt_unet_conf_ce.py:34-113), same signature and defaults.  Inputs AND targets are logits; the targets are not
detached, so the gradient reaches the network that made them through the per-pixel weight.

Per pixel, q = softmax(t), w = max q, k = arg-max t, p = softmax(x):
    L_pos = mean over {w >= threshold} of w * (logsumexp(x) - x_k)
    L_neg = mean over {softmax(t / T)_c < threshold_neg} of -[c != k'] log clamp(1 - p_c, 1e-7, 1)      (k' = arg-max of softmax(t / T))
    L_reg = 0.5 * mean p^2
    loss  = L_pos + (L_neg + L_reg  if threshold_neg > 0)

Two deviations from the reference, on every path: with no pixel over the threshold and threshold_neg == 0 the reference returns a
constant 0 without a graph, here the 0 is attached and its gradients are exact zeros; with an empty negative mask the reference's
mean() is NaN, here L_neg = 0 with zero gradient.  The fused pass evaluates 1 - p_c as the other classes' share of the softmax sum,
not by subtraction (a float32 `1 - softmax`, the reference's and the torch-op form's, is all cancellation near the clamp).  The
reference's `pass_rate` histograms, computed and discarded there, are not built; its one-hot repair branch (C inferred from the
arg-max, `.cuda()`) has no counterpart: C is the logits'."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn


def _conf_ce_torch(inputs, targets, threshold, threshold_neg, temperature_value, detach_targets=False):
    """the definition above with plain torch ops, operation by operation as the reference strings them (so `1 - softmax` IS a
    subtraction here), in the tensors' own dtype: the CPU path, the fallback, and the tests' yardstick.  The two masked means are
    sums over the mask divided by its count, so nothing waits for the device."""
    x, t = inputs, (targets.detach() if detach_targets else targets)
    q = torch.softmax(t, dim=1)
    w = q.max(1)[0]
    mask = w >= threshold
    pos = F.cross_entropy(x, torch.argmax(t, dim=1), reduction="none") * w
    loss = (pos * mask).sum() / mask.sum().clamp(min=1)
    if threshold_neg > .0:
        r = torch.softmax(t / temperature_value, dim=1)
        mask_neg = r < threshold_neg
        others = 1 - F.one_hot(torch.argmax(r, dim=1), x.shape[1]).movedim(-1, 1).type(x.dtype)
        # (a softmax of its own per term, as the reference has it: sharing one would change where the gradients are rounded)
        neg = -(others * torch.log(torch.clamp(1 - torch.softmax(x, dim=1), min=1e-7, max=1.)))
        loss = loss + (neg * mask_neg).sum() / mask_neg.sum().clamp(min=1)
        loss = loss + .5 * torch.mean(torch.softmax(x, dim=1) ** 2)
    return loss


def conf_ce_loss(inputs, targets, conf_mask=True, threshold=0.6, threshold_neg=.0, temperature_value=1, detach_targets=False):
    """the reference's conf_ce_loss(inputs, targets): both are (B, C, H, W) logits.  Float32 GPU logits of 2..4 classes take the fused
    pass (nnf.conf_ce: one launch forward, one backward, no host synchronisation); everything else the torch-op form.
    `detach_targets` (not the reference's): no gradient to the targets."""
    if not conf_mask:
        raise NotImplementedError
    from .. import nnf
    if nnf.conf_ce_supported(inputs, targets) and temperature_value > 0 and threshold_neg >= 0:
        return nnf.conf_ce(inputs, targets, threshold, threshold_neg, temperature_value, detach_targets)
    return _conf_ce_torch(inputs, targets, threshold, threshold_neg, temperature_value, detach_targets)


class ConfCELoss(nn.Module):
    def __init__(self, conf_mask=True, threshold=0.6, threshold_neg=.0, temperature_value=1, detach_targets=False):
        super().__init__()
        self.conf_mask, self.threshold, self.threshold_neg = conf_mask, threshold, threshold_neg
        self.temperature_value, self.detach_targets = temperature_value, detach_targets

    def forward(self, inputs, targets):
        return conf_ce_loss(inputs, targets, self.conf_mask, self.threshold, self.threshold_neg, self.temperature_value, self.detach_targets)


@torch.no_grad()
def unreliable_weight(target_side_logits, percent):
    """cal_unsuploss_weight (:34-48) for arg-max pseudo labels (nothing is 255 beforehand): B*H*W / #{entropy < np.percentile(entropy,
    percent)} with entropy = -sum q log(q + 1e-10) of softmax(target_side_logits).  A 0-d float32 tensor on the logits' device; on the
    GPU the entropies come from nnf.softmax_stats and the percentile from nnf.percentile, and nothing returns to the host."""
    from .. import nnf
    b, _c, h, w = target_side_logits.shape
    if nnf.softmax_stats_supported(target_side_logits):
        entropy = nnf.softmax_stats(target_side_logits, want_label=False, want_entropy=True, want_top=False)[1]
        thresh = nnf.percentile(entropy, percent)
    else:
        prob = torch.softmax(target_side_logits.float(), dim=1)
        entropy = -torch.sum(prob * torch.log(prob + 1e-10), dim=1)
        thresh = torch.as_tensor(np.percentile(entropy.cpu().numpy().flatten(), percent), device=entropy.device)
    return (b * h * w) / torch.sum(entropy < thresh)
