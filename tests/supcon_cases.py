"""Inputs and float64 restatement of the supervised contrastive loss tests (tests/golden/supcon_ref.npz, test_supcon_*): generated from
seeds on any machine, so the golden file holds only what the reference computed from them (tools/make_supcon_golden.py)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import synth

TEMPERATURE = 0.04
GOLDEN_SCALE = 0.3                                  # post-ReLU normal features at this scale keep the reference's plain exp finite (max z <= 60)
# (B, C, H, W), (Ht, Wt), label kind: the fixtures the REFERENCE module is run on (dense (HW, HW) matrices: small)
GOLDEN_CASES = [((3, 32, 16, 16), (16, 16), "three"), ((3, 16, 5, 7), (10, 14), "three"), ((4, 32, 12, 12), (12, 12), "block255")]
LABEL_KINDS = ("three", "block255", "one", "disjoint")


def features(seed: int, shape, scale: float) -> torch.Tensor:
    """post-ReLU normal features: max(N(0, 1), 0) * scale, float32"""
    n = int(np.prod(shape))
    v = np.random.Generator(np.random.PCG64(seed)).standard_normal(n)
    return torch.from_numpy((np.maximum(v, 0.0) * scale).astype(np.float32)).reshape(tuple(shape))


def targets(seed: int, b: int, ht: int, wt: int, kind: str) -> torch.Tensor:
    """(B, Ht, Wt) int64.  three: classes 0..2; block255: the same with a block of 255 in every image (a class like any other);
    one: a single class (logA == logP: the cancellation case); disjoint: image 0 holds classes 0 / 1, image 1 classes 2 / 3 (no positive pair)"""
    t = synth.labels(seed, (b, ht, wt), 3)
    if kind == "block255":
        t[:, : max(ht // 3, 1), : max(wt // 2, 1)] = 255
    elif kind == "one":
        t = torch.ones_like(t)
    elif kind == "disjoint":
        t = t.clamp(max=1)
        t[1] += 2
    elif kind != "three":
        raise ValueError(kind)
    return t


GOLDEN_SEEDS = (900, 903, 902)
# At T = 0.04 the sums are dominated by the few largest pairs.  Where the largest pair is a positive one, logA - logP is ~1e-4 and the
# gradient a cancellation (|g| is 1e-4 of either part): the reference's own float32 gradient is then 2e-3 away from float64 and no golden.
# The seeds are ones where |g| >= 0.3 of its logA part, so that the reference is good to 1e-6.


def golden_inputs(k: int):
    (b, c, h, w), (ht, wt), kind = GOLDEN_CASES[k]
    return features(GOLDEN_SEEDS[k], (b, c, h, w), GOLDEN_SCALE), targets(GOLDEN_SEEDS[k] + 20, b, ht, wt, kind)


def restate64(x: torch.Tensor, label: torch.Tensor, temperature: float = TEMPERATURE, g: float = 1.0):
    """The loss in float64 on the values `x` holds (float32 or bfloat16 -> exactly representable), dense (HW, HW) matrices, log-sum-exp form.
    The temperature is the float32 one the reference divides its float32 matrix by.  -> dict of float64 tensors / floats:
    diff = logA - logP (inf without a positive pair), loss, g1 / g2 = d (g * loss) / d x[0], x[1] as (HW, C) rows (the positive term absent
    without a positive pair), g1_all / g2_all = the logA part alone, zmax."""
    _, c, h, w = x.shape
    hw = h * w
    t = float(np.float32(temperature))
    if label.dim() == 3:
        label = label.unsqueeze(1)
    if label.shape[-2:] != x.shape[-2:]:
        label = F.interpolate(label.float(), size=(h, w), mode="nearest")
    f1, f2 = (x[k].double().permute(1, 2, 0).reshape(hw, c) for k in (0, 1))
    z = f1 @ f2.T / t
    pos = label[0].reshape(hw, 1) == label[1].reshape(1, hw)
    log_a = torch.logsumexp(z.reshape(-1), 0)
    has = bool(pos.any())
    log_p = torch.logsumexp(z[pos], 0) if has else torch.tensor(float("-inf"), dtype=torch.float64, device=x.device)
    e_all = torch.exp(z - log_a)
    e_pos = torch.where(pos, torch.exp(z - log_p), torch.zeros_like(z)) if has else torch.zeros_like(z)
    k = g / (float(hw) * float(hw)) / t
    return dict(diff=float(log_a - log_p), loss=float((log_a - log_p) / (float(hw) * float(hw))), log_a=float(log_a), log_p=float(log_p),
                g1=k * ((e_all - e_pos) @ f2), g2=k * ((e_all - e_pos).T @ f1), g1_all=k * (e_all @ f2), g2_all=k * (e_all.T @ f1), has=has,
                zmax=float(z.max()), norm=float((f1.norm(dim=1).max() * f2.norm(dim=1).max())))


def rows_of(g: torch.Tensor, k: int) -> torch.Tensor:
    """image k of a (B, C, H, W) gradient as float64 (HW, C) rows"""
    return g[k].double().permute(1, 2, 0).reshape(-1, g.shape[1])
