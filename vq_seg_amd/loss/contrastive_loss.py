"""Pixel-pair supervised contrastive loss (reference: loss/contrastive_loss.py:9-30), same class name, constructor and
`forward(x, label)`.  For images 0 and 1 of the batch, with z_ij = (f1_i . f2_j) / T over ALL pixel pairs and pos_ij = (gt1_i == gt2_j):

    loss = -log( sum_pos exp z_ij / sum_ij exp z_ij ) / (HW * HW) = (logA - logP) / (HW * HW)

Kept quirks: only the first two images enter (the batch must still hold more than two, :14); the labels are compared as they are, so
255 is a class like any other; a label map larger than the features is brought to their size by `nearest` interpolation (:18-19); the
1 / HW^2 normaliser (:29) makes the term about 1e-9 at 512 x 512 inputs -- the reference's definition, no rescaling is added.

Two deviations.  (1) The reference takes exp(z) itself, which overflows float32 at z > 88 (inf / inf = NaN at feature scales a decoder
reaches); here logA and logP are log-sum-exps -- on the GPU the fused kernels of nnf.supcon (no (HW, HW) matrix: O(HW) memory), elsewhere
torch ops over row chunks -- finite at every finite input and equal to the reference wherever that is finite.  (2) With no positive
pair the value is +inf as in the reference, but the gradient treats the positive term as absent and stays finite (the reference: NaN)."""
import torch
import torch.nn.functional as F
from torch import nn

_CHUNK_ROWS = 1024            # rows of image 0 per (chunk, HW) block of the torch-op form


def supcon_torch(x: torch.Tensor, label: torch.Tensor, temperature: float) -> torch.Tensor:
    """the torch-op form of the stabilised arithmetic: log-sum-exp over row chunks of at most (_CHUNK_ROWS, HW) pairs"""
    _, _, x_h, x_w = x.shape
    hw = x_h * x_w
    if label.dim() == 3:
        label = label.unsqueeze(1)
    if label.shape[-2:] != x.shape[-2:]:
        label = F.interpolate(label.float(), size=x.shape[-2:], mode="nearest")
    calc = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float32
    gt1, gt2 = label[0].reshape(hw), label[1].reshape(hw)
    log_all, log_pos = [], []
    with torch.autocast(device_type=x.device.type, enabled=False):      # inside a network's autocast region the product must not drop to bf16: z / T at T = 0.04
        feat_1, feat_2 = (x[k].to(calc).permute(1, 2, 0).reshape(hw, -1) for k in (0, 1))     # (HW, C)
        neg_inf = torch.full((), float("-inf"), dtype=calc, device=x.device)
        for s in range(0, hw, _CHUNK_ROWS):
            z = torch.matmul(feat_1[s:s + _CHUNK_ROWS], feat_2.transpose(0, 1)) / temperature
            pos = gt1[s:s + _CHUNK_ROWS, None] == gt2[None, :]
            log_all.append(torch.logsumexp(z.reshape(-1), dim=0))
            # the positives' log-sum-exp without a host synchronisation: -inf marks the other pairs; a chunk without a positive pair gives
            # -inf through torch.where, whose backward hands the unselected branch a zero (no log(0) is differentiated)
            zp = z.masked_fill(~pos, float("-inf"))
            top = zp.detach().max()
            top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
            total = torch.exp(zp - top).sum()
            some = total > 0
            log_pos.append(torch.where(some, top + torch.log(torch.where(some, total, torch.ones_like(total))), neg_inf))
        log_a = torch.logsumexp(torch.stack(log_all), dim=0)
        lp = torch.stack(log_pos)
        has = torch.isfinite(lp).any()
        # no positive pair anywhere: +inf as the reference, and the positive term is absent from the gradient (where cuts the NaN of lse(-inf, ...))
        log_p = torch.where(has, torch.logsumexp(torch.where(has, lp, torch.zeros_like(lp)), dim=0), neg_inf)
        return (log_a - log_p) / (x_h * x_w * x_h * x_w)


class SupConLoss(nn.Module):
    def __init__(self, temperature=0.04):
        super().__init__()
        self.temperature = temperature

    def forward(self, x: torch.Tensor, label: torch.Tensor):
        assert x.shape[0] > 2, "supervised contrasitve loss can be computed when batch size is larger than 2"
        from .. import nnf
        if nnf.supcon_supported(x, label):
            return nnf.supcon(x, label, self.temperature)    # HIP: fused forward / backward, no (HW, HW) matrix
        return supcon_torch(x, label, self.temperature)
