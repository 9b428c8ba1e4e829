"""Seeded inputs, the float64 restatement and the margin rule of the confidence-weighted CPS loss tests (loss.conf_ce_loss,
nnf.conf_ce / conf_ce_pair; tools/make_conf_ce_golden.py writes tests/golden/conf_ce_ref.npz from the golden cases here).

The loss takes decisions that are discontinuous in the logits -- the confidence mask w >= threshold, the negative mask
r_c < threshold_neg, the arg-max, the clamp of 1 - p -- and its value is a handful of GLOBAL sums, so one pixel that a float32
evaluation decides the other way than float64 would move a sum by a whole term, and no exclusion of that pixel can mend a sum.
Every case is therefore made margin-clean when it is built: a pixel that violates one of

    |w - threshold| > 1e-5      |r_c - threshold_neg| > 1e-5 (threshold_neg > 0)      top-two gap of the target logits > 1e-4
    1 - p_c outside [5e-8, 2e-7] (the clamp's edge at 1e-7)

in float64, with EITHER tensor in the target's role (the pair form uses both), is redrawn from the next seed until none remains.
The number of redrawn pixels is recorded and must stay under 1 % of the case (tests/test_conf_ce_cpu.py)."""
import functools

import torch

from tests import synth

# name -> (threshold, threshold_neg, temperature, logit scale)
CASES = {
    "ref": (0.6, 0.0, 1.0, 8.0),            # the reference trainer's call
    "neg": (0.6, 0.1, 1.0, 8.0),
    "neg_t2": (0.6, 0.1, 2.0, 8.0),
    "all_t05": (0.0, 0.05, 0.5, 8.0),
    "m0": (0.99999, 0.0, 1.0, 1.0),         # scale 1: the top probability stays below 0.89, so M == 0
    # Mn == 0: no r_c is below 1e-30.  Scale 4, so that every r_c >= exp(-8) / 4 = 8e-5 keeps the 1e-5 margin to the threshold (at scale
    # 8 r_c reaches 1e-7: on the right side of 1e-30 by 23 orders of magnitude, but inside the margin as the rule words it)
    "mn0": (0.6, 1e-30, 1.0, 4.0),
    # logits in (-12, 12): scale 8, and on a seeded 5 % of the pixels of each tensor one class at 11 + U(-1, 1), the others at
    # -11 + U(-1, 1): there 1 - p is below 1e-9, far under the clamp, so clamped elements exist at every shape and carry no gradient
    "clamp": (0.6, 0.1, 1.0, 8.0),
}
GOLDEN_SHAPE = (2, 3, 8, 12)
GOLDEN_SCALE = 3.0                           # 1 - p >= 2e-3: the reference's float64 `1 - softmax` keeps 13 digits there
GOLDEN_CASES = ("ref", "neg", "neg_t2", "all_t05", "m0", "mn0")
GOLDEN_PERCENTS = (80.0, 93.5)


def _draw(seed, shape, scale, spikes):
    x = synth.uniform(seed, shape, -scale, scale)
    if spikes:
        b, c, h, w = shape
        pick = synth.uniform(seed + 101, (b, 1, h, w)) < 0.05
        cls = synth.labels(seed + 102, (b, 1, h, w), c)
        spike = torch.where(torch.arange(c).view(1, c, 1, 1) == cls, 11.0, -11.0) + synth.uniform(seed + 103, shape, -1.0, 1.0)
        x = torch.where(pick, spike, x)
    return x


def _violations(x, t, thr, thrn, temp):
    """(B, H, W) bool: pixels of the direction x <- t that are within a margin, in float64"""
    x, t = x.double(), t.double()
    q = torch.softmax(t, dim=1)
    top2 = t.topk(2, dim=1).values
    bad = ((q.amax(dim=1) - thr).abs() <= 1e-5) | (top2[:, 0] - top2[:, 1] <= 1e-4)
    if thrn > 0:
        bad |= ((torch.softmax(t / temp, dim=1) - thrn).abs() <= 1e-5).any(dim=1)
    u = one_minus_softmax(x)
    return bad | ((u >= 5e-8) & (u <= 2e-7)).any(dim=1)


def one_minus_softmax(x):
    """1 - softmax(x, dim=1) as (sum of the other classes' exponentials) / (sum of all): no cancellation"""
    e = torch.exp(x - x.amax(dim=1, keepdim=True))
    c = x.shape[1]
    rest = torch.stack([sum(e[:, j] for j in range(c) if j != i) for i in range(c)], dim=1)
    return rest / e.sum(dim=1, keepdim=True)


def build(seed, shape, thr, thrn, temp, scale, spikes=False):
    """-> a, b (float32, margin-clean in both directions) and the number of redrawn pixels"""
    a, b = _draw(seed, shape, scale, spikes), _draw(seed + 500, shape, scale, spikes)
    redrawn = None
    for k in range(1, 50):
        bad = _violations(a, b, thr, thrn, temp) | _violations(b, a, thr, thrn, temp)
        if not bool(bad.any()):
            break
        redrawn = bad if redrawn is None else redrawn | bad
        na, nb = _draw(seed + 1000 * k, shape, scale, spikes), _draw(seed + 500 + 1000 * k, shape, scale, spikes)
        a, b = torch.where(bad[:, None], na, a), torch.where(bad[:, None], nb, b)
    else:
        raise AssertionError("margin-clean inputs not reached")
    return a, b, 0 if redrawn is None else int(redrawn.sum())


@functools.lru_cache(maxsize=None)
def inputs(name, shape):
    """the case `name` at (B, C, H, W): a, b, redrawn pixels"""
    thr, thrn, temp, scale = CASES[name]
    seed = 7000 + 37 * sorted(CASES).index(name) + sum(shape)
    return build(seed, tuple(shape), thr, thrn, temp, scale, spikes=name == "clamp")


@functools.lru_cache(maxsize=None)
def golden_inputs(name):
    """the golden case `name`: moderate logits at GOLDEN_SHAPE, every class the arg-max of both tensors somewhere (the
    reference's one_hot infers the class count from the largest arg-max)"""
    thr, thrn, temp, scale = CASES[name]
    scale = min(scale, GOLDEN_SCALE)
    a, b, redrawn = build(9000 + 37 * sorted(CASES).index(name), GOLDEN_SHAPE, thr, thrn, temp, scale)
    for v in (a, b):
        assert sorted(v.argmax(dim=1).unique().tolist()) == list(range(GOLDEN_SHAPE[1]))
    return a, b, redrawn


def params(name):
    return CASES[name][:3]


def restate(x, t, thr, thrn, temp, detach_targets=False, parts=None):
    """the definition in float64 (differentiable with respect to x and t): masks and arg-maxes are constants, a mean over an empty
    mask is 0.  `parts`: a dict that receives the sums and counts."""
    x, t = x.double(), t.double()
    if detach_targets:
        t = t.detach()
    n = x.numel()
    q = torch.softmax(t, dim=1)
    w, _ = q.max(dim=1)
    k = t.argmax(dim=1)                                          # first maximum
    pos = w * (torch.logsumexp(x, dim=1) - x.gather(1, k[:, None])[:, 0])
    mask = (w >= thr).detach()
    m = int(mask.sum())
    s_pos = (pos * mask).sum()
    loss = s_pos / m if m else s_pos * 0.0
    s_neg, s_p2, mn = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64), 0
    if thrn > 0:
        r = torch.softmax(t.detach() / temp, dim=1)
        kn = r.argmax(dim=1)
        other = torch.arange(x.shape[1]).view(1, -1, 1, 1) != kn[:, None]
        u = torch.clamp(one_minus_softmax(x), min=1e-7, max=1.0)
        neg_mask = r < thrn
        mn = int(neg_mask.sum())
        s_neg = (-(torch.log(u) * other) * neg_mask).sum()
        s_p2 = (torch.softmax(x, dim=1) ** 2).sum()
        loss = loss + (s_neg / mn if mn else s_neg * 0.0) + 0.5 * s_p2 / n
    if parts is not None:
        parts.update(sum_pos=float(s_pos), sum_neg=float(s_neg), sum_p2=float(s_p2), m=m, mn=mn, loss=float(loss))
    return loss


def restate_grads(x, t, thr, thrn, temp, detach_targets=False):
    """-> loss, d loss / d x, d loss / d t (zeros when detached) in float64"""
    xv, tv = x.double().clone().requires_grad_(True), t.double().clone().requires_grad_(True)
    loss = restate(xv, tv, thr, thrn, temp, detach_targets)
    gx, gt = torch.autograd.grad(loss, (xv, tv), allow_unused=True)
    return loss.detach(), gx, torch.zeros_like(tv) if gt is None else gt


def unreliable_weight64(logits, percent):
    """B*H*W / #{entropy < percentile}: the entropies in float32 as the reference takes them, np.percentile's interpolation"""
    import numpy as np
    prob = torch.softmax(logits.float(), dim=1)
    entropy = -torch.sum(prob * torch.log(prob + 1e-10), dim=1)
    thresh = np.percentile(entropy.numpy().flatten(), percent)
    b, _c, h, w = logits.shape
    return b * h * w / float((entropy < float(thresh)).sum())
