"""Direct parity of the older loss kernels of csrc/loss_kernels.hip -- the Dice / Dice+CE sums (forward, fold, backward),
softmax_stats, both prototype losses and cps_loss_combine -- through the C ABI (nnf where the ABI takes pointer tables) against
plain float64 computations of the same operations on the CPU, on exactly the values the kernels receive.

Reference.  The float64 arithmetic is oracle/torch_ref.py's (dice_loss, prototype_loss_v1 / _v2, _margin_terms) run in float64.
Where a check needs per-image sums or per-row terms that those functions do not expose, they are written out below
(`dice_pieces`, `proto_ll`, `proto_closed`, `combine_ref`); tests/test_loss_restatements_cpu.py ties every one of them to
torch_ref's scalars on the golden inputs, so this file's references hang on tests/golden/prototype.npz and losses_metrics.npz.

Bars.  None is fitted to the kernels' output.
  * exact quantities (labels, pixel counts, zeros on ignored pixels, untouched bytes, repeated calls): bit for bit;
  * per-element outputs (Dice logit gradient, entropy, top probability, gx, the combine kernel's gradients):
    |got - ref| <= k u S (+ half a bf16 ulp), u = 2^-24, S the float64 sum of the absolute values of the terms that make the
    element, k the fp32 roundings of the kernel's expression counted from the source next to each check; expf / logf / sqrtf
    count 2 (1 ulp, the HIP math API's documented bound), and expf(z - mx) adds |z - mx| (the rounding of its argument);
  * reduced outputs (inter, sets, ce[:, 0], the prototype loss, the combine kernel's scalars): 2e-6 relative
    (test_loss_gpu.py, test_focal_gpu.py); the prototype gradient: 2e-5 of the tensor scale (SUM_BAR, test_nn_kernels_gpu.py).
Measured errors against these bars: profiles/loss_parity.md."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from tests import synth
from tests.test_nn_kernels_gpu import BF16, F32, SUM_BAR, U, check_sum, dev, half_ulp_bf16, lib, nan_like, ok, ptr, rnd, stream

pytestmark = pytest.mark.gpu

LOSS_BAR = 2e-6                   # loss values against fp64, relative (test_loss_gpu.py, test_focal_gpu.py)
PX_PER_BLOCK = 4096               # DICE_PX_PER_BLOCK (csrc/loss_kernels.h)
IGNORE, NO_IGNORE = 255, -(1 << 62)


def note(family, what, err, bar):
    """every check prints its error and its bar before it asserts (pytest -s: the source of profiles/loss_parity.md)"""
    print(f"[{family}] {what}: error {err:.3e}, bar {bar:.3e}" + (f" ({err / bar:.2f} of it)" if bar > 0 else ""))


def check_rel(got, ref, what, family, bar=LOSS_BAR, floor=0.0):
    """reduced forward sums, entry by entry: |got - ref| <= max(2e-6 |ref|, floor)"""
    got = got.detach().double().cpu().reshape(ref.shape)
    lim = torch.maximum(bar * ref.abs(), torch.as_tensor(floor, dtype=torch.float64).expand(ref.shape))
    err, lim = (got - ref).abs().reshape(-1), lim.reshape(-1)
    i = int((err / lim.clamp_min(1e-300)).argmax())
    note(family, what, float(err[i]), float(lim[i]))
    assert bool((err <= lim).all()), f"{what}: entry {i}: got {got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r}"


def checked(got, ref, S, k, dtype, what, family, extra=None):
    """the per-element bound of test_nn_kernels_gpu.check -- |got - ref| <= k u S (+ extra) (+ half a bf16 ulp at the magnitude the fp32
    result can reach) -- which also prints and returns the worst error as a share of the bound"""
    got = got.detach().double().cpu().reshape(ref.shape)
    bound = k * U * S.double() + (0 if extra is None else extra)
    if dtype == BF16:
        bound = bound + half_ulp_bf16(ref.abs() + bound)
    err = (got - ref).abs()
    ratio = (err.nan_to_num(float("inf")) / bound.clamp_min(1e-300)).reshape(-1)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    note(family, what, worst, 1.0)
    bad = ~(err <= bound)                                              # NaN counts as a failure
    if bad.any():
        i = int(ratio.argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat index {i}: "
                             f"got {got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r} bound {bound.reshape(-1)[i].item():.3e}")
    return worst


# ==================================================================================================================
# float64 restatements (CPU).  Tied to oracle/torch_ref.py by tests/test_loss_restatements_cpu.py.
# ==================================================================================================================
def dice_pieces(z, target, ignore):
    """loss/dice_loss.py:12-26 per image, as torch_ref.dice_loss states it: z (B, C, HW) float64, target (B, HW) int64 ->
    inter (B, C), sets (B, C), ce (B, 2) = (sum of -log softmax[target] over kept pixels, their number)"""
    c = z.shape[1]
    keep = target != ignore
    zz = z * keep[:, None, :]                                  # ignored pixels: ZERO logits ...
    t = target * keep                                          # ... and class-0 targets
    onehot = F.one_hot(t, c).permute(0, 2, 1).double()
    prob = torch.softmax(zz, dim=1)
    inter = (prob * onehot).sum(dim=2)
    sets = (prob + onehot).sum(dim=2)
    nll = -(torch.log_softmax(zz, dim=1) * onehot).sum(dim=1) * keep
    ce = torch.stack([nll.sum(dim=1), keep.sum(dim=1).double()], dim=1)
    return inter, sets, ce


def dice_ce_floor(z, target, ignore):
    """what the counted roundings allow ce[:, 0] per image, whatever the number of pixels.  dice_pixel: nll = logf(sum) + mx - zt per kept
    pixel.  sum's own relative error (its terms' shares and C - 1 additions, softmax_rho) becomes an absolute one of the logarithm;
    logf: 2 on |log sum|; the addition: 1 on |log sum| + |mx|; the subtraction: 1 on |log sum| + |mx| + |zt|; the cast of the image's
    double sum: 1 on the entry:   u sum_kept [ share + (C - 1) + 4 |log sum| + 2 |mx| + |zt| ] + u |ce|.
    It is above 2e-6 of the entry only where the entry is a few pixels whose target is the confident maximum (HW = 1: an nll of 1e-8
    is below what fp32 resolves in that expression, the kernel's as nn.CrossEntropyLoss's)."""
    keep = target != ignore
    mx = z.amax(dim=1)
    zt = z.gather(1, (target * keep)[:, None, :])[:, 0]
    lsum = torch.log(torch.exp(z - mx[:, None]).sum(dim=1))
    share = softmax_rho(z)[2][:, 0]
    nll = (lsum + mx - zt) * keep
    per_px = (share + (z.shape[1] - 1) + 4 * lsum.abs() + 2 * mx.abs() + zt.abs()) * keep
    return U * (per_px.sum(dim=1) + nll.sum(dim=1).abs())


def dice_sum_floors(z, target, ignore):
    """what the counted roundings allow inter and sets per image and class, whatever the number of pixels -> (inter's, sets').  Every
    pixel's p_c carries rho_c roundings (softmax_rho; |z - mx| u of it is expf's argument), and a probability below fp32's normal range
    has an absolute spacing and may be flushed (2^-126 a pixel).
      inter sums p_c * onehot (exact) over the pixels whose target is c, in double; the cast of the sum: 1 on the entry:
          u sum_px onehot p_c rho_c + u inter + (number of target pixels) 2^-126
      sets sums p_c + onehot over all pixels: that addition and the cast 2 more:
          u sum_px p_c (rho_c + 2) + u (number of target pixels) + HW 2^-126.
    Each is above 2e-6 of its entry only where a few pixels with |z - mx| ~ 50 and more make the entry (HW = 1)."""
    keep = target != ignore
    zz = z * keep[:, None, :]
    onehot = F.one_hot(target * keep, z.shape[1]).permute(0, 2, 1).double()
    rho, p, _ = softmax_rho(zz)
    n_t = onehot.sum(dim=2)
    f_inter = U * ((onehot * p * rho).sum(dim=2) + (onehot * p).sum(dim=2)) + n_t * 2.0 ** -126
    f_sets = U * ((p * (rho + 2)).sum(dim=2) + n_t) + z.shape[2] * 2.0 ** -126
    return f_inter, f_sets


def dice_from_pieces(inter, sets):
    """dice_loss.py:27-37: 1 - mean_c mean_b 2 inter / (sets + 1e-6)"""
    return 1 - (2 * inter / (sets + 1e-6)).mean(dim=0).mean()


def softmax_rho(zz):
    """fp32 roundings (units of u) in p_c = expf(z_c - mx) / sum, relative to p_c, from dice_pixel / softmax_stats_kernel:
    e_c = expf(z_c - mx): the subtraction's rounding moves the argument by u |z_c - mx| (relative |z_c - mx| u in e_c), expf 2;
    sum: C - 1 additions, and its terms' own errors, weighted by their share; inv = 1 / sum: 1; p_c = e_c * inv: 1."""
    c = zz.shape[1]
    d = (zz - zz.amax(dim=1, keepdim=True)).abs()
    p = torch.softmax(zz, dim=1)
    share = (p * (d + 2)).sum(dim=1, keepdim=True)
    return d + 2 + share + (c - 1) + 2, p, share


def dice_grad_bound(z, target, ignore, gi, gs, gce):
    """bound / u of dice_bwd_kernel's  g = fma(gce, p_c - oh, p_c * (dp_c - dotp)),  dp_c = gs_c + gi_c oh,  dotp = sum_c dp_c p_c (C fmas):
       p_c (|dp_c| + D) (rho_c + 4)        p_c's roundings; dp_c: 1, the subtraction: 1, the product: 1, the final fma: 1;  D = sum |dp p|
     + p_c sum_c' |dp_c'| p_c' (C + rho_c')    dotp's own error: C fmas on D, and the p's inside it
     + |gce| (p_c rho_c + 2 (p_c + oh))        the CE part: p_c's roundings, p_c - oh: 1, the fma: 1"""
    c = z.shape[1]
    keep = target != ignore
    zz = z * keep[:, None, :]
    onehot = F.one_hot(target * keep, c).permute(0, 2, 1).double()
    rho, p, _ = softmax_rho(zz)
    dp = (gs[:, :, None] + gi[:, :, None] * onehot).abs()
    D = (dp * p).sum(dim=1, keepdim=True)
    S = p * (dp + D) * (rho + 4) + p * (dp * p * (c + rho)).sum(dim=1, keepdim=True)
    if gce is not None:
        S = S + gce.abs()[:, None, None] * (p * rho + 2 * (p + onehot))
    return S * keep[:, None, :]


def dice_grad_ref(z, target, ignore, gi, gs, gce):
    """d (sum g_inter inter + sum g_sets sets + sum g_ce[:, 0] ce[:, 0]) / d z by autograd through dice_pieces"""
    x = z.clone().requires_grad_(True)
    inter, sets, ce = dice_pieces(x, target, ignore)
    y = (gi * inter).sum() + (gs * sets).sum()
    if gce is not None:
        y = y + (gce * ce[:, 0]).sum()
    return torch.autograd.grad(y, x)[0]


def proto_ll(x, proto, labels, variant, margin, scale, easy):
    """per-row log-likelihood of ReliablePrototypeLoss (variant 1, prototype.py:556-593) / ReliablePrototypeLossv2 (:844-868) as
    torch_ref.prototype_loss_v1 / _v2 state them, float64, differentiable: x (M, C), proto (K, C) ALREADY L2-normalised (what the
    kernel receives), labels (M,) -> ll (M,); the loss is -mean(ll * w)"""
    rows = F.normalize(x, p=2, dim=-1)
    cosine = F.linear(rows, proto)
    phi = R._margin_terms(cosine, margin, easy)
    if variant == 1:
        onehot = torch.zeros(x.shape[0], proto.shape[0], dtype=torch.float64).scatter_(1, labels[:, None], 1.0) + 1e-6
        if margin != 0:
            cosine = (onehot * phi) + ((1.0 - onehot) * cosine)
        cosine = scale * cosine
        positive = torch.exp(torch.sum(cosine * onehot, dim=-1))
    else:
        hit = F.one_hot(labels, proto.shape[0]).bool()
        cosine = scale * torch.where(hit, cosine * phi, cosine)
        positive = torch.exp(cosine.gather(1, labels[:, None])[:, 0])
    total = torch.sum(torch.exp(cosine), dim=-1)
    return torch.log((positive / (total + 1e-7)) + 1e-7)


def proto_ref(x, proto, labels, w, g, variant, margin, scale, easy):
    """(loss, d (g loss) / d x, d (g loss) / d proto), float64, by autograd through proto_ll"""
    xx, pp = x.clone().requires_grad_(True), proto.clone().requires_grad_(True)
    loss = -torch.mean(proto_ll(xx, pp, labels, variant, margin, scale, easy) * w)
    gx, gp = torch.autograd.grad(loss * g, (xx, pp))
    return loss.detach(), gx, gp


def proto_closed(x, proto, labels, w, g, variant, margin, scale, easy, dcos=None, dinner=0.0, dzt=None):
    """the closed form the kernel evaluates (row_terms, proto_bwd_kernel), float64, with room to move what fp32 rounds on the way:
    `dcos` (M, K) is added to the cosines, `dinner` to 1 - cos^2 under the root, `dzt` (M,) to the target's z before the scale.
    -> gx (M, C); S (M, C): the sum of the absolute values of gx's terms; the target's |phi| terms; the cosines; Sd (M, C): S with
    dll_dz replaced by the sum of the two terms it is the difference of"""
    m, k = x.shape[0], proto.shape[0]
    cm, sm = math.cos(margin), math.sin(margin)
    th, mm = math.cos(math.pi - margin), math.sin(math.pi - margin) * margin
    inv_n = 1.0 / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    r = x * inv_n
    cos = r @ proto.t()
    if dcos is not None:
        cos = cos + dcos
    hit = F.one_hot(labels, k).bool()
    raw = 1.0 - cos * cos + dinner
    sine = raw.clamp(0, 1).sqrt()
    dsine = torch.where((raw > 0) & (raw <= 1), -cos / sine.clamp_min(1e-300), torch.zeros_like(cos))
    sel = cos > 0 if easy else cos > th
    f = torch.where(sel, cos * cm - sine * sm, cos if easy else cos - mm)
    df = torch.where(sel, cm - sm * dsine, torch.ones_like(cos))
    f_abs = torch.where(sel, (cos * cm).abs() + (sine * sm).abs(), cos.abs() + (0.0 if easy else abs(mm)))
    df_abs = torch.where(sel, abs(cm) + (sm * dsine).abs(), torch.ones_like(cos))
    if variant == 1:
        ohe = hit.double() + 1e-6
        if margin != 0:
            z, dz, dz_abs = ohe * f + (1 - ohe) * cos, ohe * df + (1 - ohe), ohe * df_abs + (1 - ohe).abs()
        else:
            z, dz, dz_abs = cos, torch.ones_like(cos), torch.ones_like(cos)
    else:
        ohe = hit.double()
        z = torch.where(hit, cos * f, cos)
        dz = torch.where(hit, f + cos * df, torch.ones_like(cos))
        dz_abs = torch.where(hit, f_abs + cos.abs() * df_abs, torch.ones_like(cos))
    if dzt is not None:
        z = z + hit * dzt[:, None]
    z, dz, dz_abs = z * scale, dz * scale, dz_abs * scale
    pos = torch.exp((z * ohe).sum(dim=1, keepdim=True))
    den = torch.exp(z).sum(dim=1, keepdim=True) + 1e-7
    q = pos / den + 1e-7
    dll_dz = (pos * ohe / den - pos * torch.exp(z) / (den * den)) / q
    krow = (-g * w / m)[:, None]
    gcos = krow * dll_dz * dz
    gx = (gcos @ proto - (gcos * cos).sum(dim=1, keepdim=True) * r) * inv_n
    gabs = (krow * dll_dz).abs() * dz_abs
    S = (gabs @ proto.abs() + (gabs * cos.abs()).sum(dim=1, keepdim=True) * r.abs()) * inv_n
    dabs = krow.abs() * ((pos * ohe / den + pos * torch.exp(z) / (den * den)) / q) * dz_abs          # the two terms dll_dz is the difference of
    Sd = (dabs @ proto.abs() + (dabs * cos.abs()).sum(dim=1, keepdim=True) * r.abs()) * inv_n
    return gx, S, f_abs.gather(1, labels[:, None])[:, 0], cos, Sd


def proto_gx_bound(x, proto, labels, w, g, variant, margin, scale, easy):
    """-> (k, S, extra) for check(): |gx - ref| <= k u S + extra.
    k, from proto_bwd_kernel: gc_c = (float)(...): 1; gs: K fmas; u_i * inv_n: 1; gs * r_i: 1; K fmas; the final product: 1; inv_n
    (n2: C fmas of positive terms, sqrtf 2, halved by the root; 1 / n: 1 -> C / 2 + 2) enters twice: C + 4; phi_of and dphi_of of the
    target (c * cos_m, sqrtf 2, * sin_m, the difference; the quotient, sqrtf 2, * sin_m, the difference; cs * ph; cos_m and sin_m
    themselves arrive as floats: 2): 14  ->  k = 2 K + C + 22.
    extra, what the roundings BEFORE the margin and the softmax do to gx (they do not enter as a multiple of a term of gx: 1 - c^2
    cancels near |c| = 1, the softmax's curvature grows with the scale).  The fp64 closed form is evaluated at the corners of the box
        cos_c +- (1.5 C + 3) u sum_i |r_i p_ci|     C fmas of the dot product, times inv_n (C / 2 + 2) and the product (1)
        1 - c^2 +- 2 u                              c * c: 1 (c^2 <= 1), the difference: 1 (<= 1)
        z_t +- 6 u f_abs                            phi_of's five roundings on its terms' absolute sum, and cs * ph
    and the largest deviation from the centre is allowed on top (exact for a linear dependence: max over signs of
    |sum s_j a_j d_j| = sum |a_j| d_j).  Last, dll_dz = (pos oh / den - pos exp(z) / den^2) / q is a difference taken in DOUBLE, by the
    kernel and by the reference alike; where the target dominates (scale 30: exp(z_t) ~ 1e16) it cancels down to double's own
    rounding, so both get 10 roundings of 2^-53 (exp 2, the two quotients 2 + 3, the difference, / q, the product) on Sd."""
    k_, c_ = proto.shape
    gx0, S, f_abs, _, Sd = proto_closed(x, proto, labels, w, g, variant, margin, scale, easy)
    r = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    dcos = (1.5 * c_ + 3) * U * (r.abs() @ proto.abs().t())
    extra = 20 * 2.0 ** -53 * Sd
    dev0 = torch.zeros_like(gx0)
    for signs in itertools.product((-1.0, 1.0), repeat=k_ + 2):
        s = torch.tensor(signs[:k_], dtype=torch.float64)
        gx1 = proto_closed(x, proto, labels, w, g, variant, margin, scale, easy, dcos * s, signs[k_] * 2 * U, signs[k_ + 1] * 6 * U * f_abs)[0]
        dev0 = torch.maximum(dev0, (gx1 - gx0).abs())
    return 2 * k_ + c_ + 22, S, extra + dev0, gx0


def combine_ref(terms, n_sup, cps_w, ce_w, eps, commits, com_w, protos, pro_w):
    """the CPS step's total (train_vqreptunet1x1v2.py:165-192; dice_loss.py:27-37) from float64 leaves -> (total, stats)"""
    def scalar(t):
        v = 1 - (2 * t[0] / (t[1] + eps)).mean(dim=0).mean()
        return v if len(t) == 2 else ce_w * (t[2][:, 0].sum() / t[2][:, 1].sum()) + v
    vals = [scalar(t) for t in terms]
    zero = torch.zeros((), dtype=torch.float64)
    sup = sum(vals[:n_sup], zero)
    cps = sum(vals[n_sup:], zero)
    com = sum((sum(c[l] for c in commits) * com_w for l in range(commits[0].numel())), zero) if commits else zero
    pro = sum(protos, zero) * pro_w
    total = sup + cps_w * cps + com + pro
    return total, torch.stack([total, com, pro, cps] + vals)


# ==================================================================================================================
# 1 + 2. Dice and Dice+CE sums
# ==================================================================================================================
DICE_B = 3
DICE_HW = [1, 255, 257, 4095, 4096, 4097, 3 * 4096 + 5]
LAYOUTS = ["nchw", "nhwc", "window"]


@functools.lru_cache(maxsize=None)
def dice_inputs(c, hw):
    """image 0: ~20 % ignored pixels, image 1: every pixel ignored, image 2: none.  Logits +-8; the last (up to) 16 pixels -- inside the
    last, short span -- scaled by 6 (|z| up to 48: nll up to ~96)."""
    seed = 7000 + 1000 * c + hw % 997
    z = synth.uniform(seed, (DICE_B, c, hw), -8.0, 8.0)
    last_span = (hw - 1) // PX_PER_BLOCK * PX_PER_BLOCK
    z[:, :, max(last_span, hw - 16):] *= 6.0
    clean = synth.labels(seed + 1, (DICE_B, hw), c)
    t = clean.clone()
    t[0][synth.uniform(seed + 2, (hw,)) < 0.2] = IGNORE
    t[1] = IGNORE
    g = [synth.uniform(seed + 3 + i, s, -1.5, 1.5) for i, s in enumerate([(DICE_B, c), (DICE_B, c), (DICE_B, 2)])]
    return z, t, clean, g


def place(z, layout, fill=None):
    """-> (storage on the device, pointer of element (0, 0, 0), (sb, sc, sp), index of the window in the storage).  `fill`: the storage
    holds this value and no logits (an output buffer)."""
    b, c, hw = z.shape
    if layout == "nchw":
        host, strides, win = z.clone(), (c * hw, hw, 1), (slice(None), slice(None), slice(None))
    elif layout == "nhwc":
        host, strides, win = z.permute(0, 2, 1).contiguous(), (c * hw, 1, c), None
    else:                                                       # a channel window of a (B, C + 2, HW) tensor
        host = synth.uniform(99, (b, c + 2, hw), -3.0, 3.0)
        host[:, 1:c + 1] = z
        strides, win = ((c + 2) * hw, hw, 1), (slice(None), slice(1, c + 1), slice(None))
    store = host.to(dev()) if fill is None else torch.full(host.shape, fill, dtype=F32, device=dev())
    base = store.data_ptr() + (hw * 4 if layout == "window" else 0)
    return store, base, strides, win


def unplace(store, layout, win):
    return store.permute(0, 2, 1) if layout == "nhwc" else store[win]


def dice_forward(z, t_dev, layout, ignore, with_ce, ws_bytes=None, guard=0):
    L = lib()
    b, c, hw = z.shape
    store, base, (sb, sc, sp), _ = place(z, layout)
    need = L.vqseg_dice_workspace_bytes(b, c, hw)
    assert need == b * ((hw + PX_PER_BLOCK - 1) // PX_PER_BLOCK) * (2 * c + 2) * 8
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev())
    inter, sets = nan_like((b, c), F32), nan_like((b, c), F32)
    ce = nan_like((b, 2), F32) if with_ce else None
    nbytes = need if ws_bytes is None else ws_bytes
    if with_ce:
        rc = L.vqseg_dice_ce_sums_forward_f(base, sb, sc, sp, t_dev.data_ptr(), b, c, hw, ignore, ws.data_ptr(), nbytes, inter.data_ptr(),
                                            sets.data_ptr(), ce.data_ptr(), stream())
    else:
        rc = L.vqseg_dice_sums_forward_f(base, sb, sc, sp, t_dev.data_ptr(), b, c, hw, ignore, ws.data_ptr(), nbytes, inter.data_ptr(),
                                         sets.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, inter, sets, ce, ws


@pytest.mark.parametrize("hw", DICE_HW)
@pytest.mark.parametrize("c", [2, 3, 4])
def test_dice_sums_forward(c, hw):
    """inter, sets and ce[:, 0] per image (and class): 2e-6 of the entry, or where larger each output's own counted roundings
    (dice_sum_floors, dice_ce_floor), asserted below to be the larger only at HW = 1; ce[:, 1] (a count) exact.  The fully ignored
    image: zero logits and class-0 targets give inter[b][0] = HW / C = sets[b][0] - HW (sets / 2 - HW / 2 would be HW / (2 C); the
    fp64 restatement, pinned to the golden file, gives HW / C), the other classes inter = 0 and sets = HW / C, ce[b] == (0, 0)."""
    z, t, clean, _ = dice_inputs(c, hw)
    zd = z.double()
    for ignore, tgt in ((IGNORE, t), (NO_IGNORE, clean)):
        ref = dice_pieces(zd, tgt, ignore)
        ce_floor, (i_floor, s_floor) = dice_ce_floor(zd, tgt, ignore), dice_sum_floors(zd, tgt, ignore)
        if hw > 1:                                              # the issue's 2e-6 governs every entry that is a sum of pixels
            for fl, r in ((i_floor, ref[0]), (s_floor, ref[1]), (ce_floor, ref[2][:, 0])):
                assert bool((fl <= LOSS_BAR * r.abs())[r != 0].all()), (c, hw, ignore)
        t_dev = tgt.to(dev())
        for layout in (LAYOUTS if ignore == IGNORE else ["nchw"]):
            for with_ce in (False, True):
                rc, inter, sets, ce, _ = dice_forward(z, t_dev, layout, ignore, with_ce)
                ok(rc)
                tag = f"C{c} HW{hw} {layout} ignore {ignore != NO_IGNORE} ce {with_ce}"
                check_rel(inter, ref[0], f"inter {tag}", "dice forward", floor=i_floor)
                check_rel(sets, ref[1], f"sets {tag}", "dice forward", floor=s_floor)
                if with_ce:
                    check_rel(ce[:, 0], ref[2][:, 0], f"ce sum {tag}", "dice forward", floor=ce_floor)
                    assert torch.equal(ce[:, 1].cpu().double(), ref[2][:, 1]), f"kept-pixel count {tag}"
                if ignore == IGNORE:
                    i1, s1 = inter[1].double().cpu(), sets[1].double().cpu()
                    assert abs(i1[0] - hw / c) <= LOSS_BAR * hw / c and abs(i1[0] - (s1[0] - hw)) <= LOSS_BAR * s1[0], tag
                    assert bool((i1[1:] == 0).all()) and bool(((s1[1:] - hw / c).abs() <= LOSS_BAR * hw / c).all()), tag
                    if with_ce:
                        assert ce[1].tolist() == [0.0, 0.0], tag


@pytest.mark.parametrize("hw", [1, 4097])
def test_dice_workspace_size_is_enough_and_enforced(hw):
    """the size vqseg_dice_workspace_bytes returns is enough (a guard band behind it keeps its pattern) and one byte less is refused"""
    c = 4
    z, t, _, _ = dice_inputs(c, hw)
    need = lib().vqseg_dice_workspace_bytes(DICE_B, c, hw)
    rc, inter, _, _, ws = dice_forward(z, t.to(dev()), "nchw", IGNORE, True, guard=256)
    ok(rc)
    assert bool((ws[need:] == 0xA5).all()) and bool(torch.isfinite(inter).all())
    rc, inter, sets, ce, _ = dice_forward(z, t.to(dev()), "nchw", IGNORE, True, ws_bytes=need - 1)
    assert rc != 0 and bool(torch.isnan(inter).all()) and bool(torch.isnan(ce).all())


@pytest.mark.parametrize("hw", [257, 4097, 3 * 4096 + 5])
@pytest.mark.parametrize("c", [2, 3, 4])
def test_dice_sums_backward(c, hw):
    """every element of the logit gradient against autograd through the fp64 restatement, with random cotangents of both signs; the
    bound: dice_grad_bound.  Ignored pixels exactly 0; outside a channel window nothing is written."""
    L = lib()
    z, t, _, (gi, gs, gce) = dice_inputs(c, hw)
    zd, t_dev = z.double(), t.to(dev())
    gid, gsd, gced = gi.to(dev()), gs.to(dev()), gce.to(dev())
    ignored = (t == IGNORE)[:, None, :].expand(-1, c, -1)
    for with_ce in (True, False):
        g_ce = gce[:, 0].double() if with_ce else None
        ref = dice_grad_ref(zd, t, IGNORE, gi.double(), gs.double(), g_ce)
        S = dice_grad_bound(zd, t, IGNORE, gi.double(), gs.double(), g_ce)
        for layout in LAYOUTS:
            store, base, (sb, sc, sp), _ = place(z, layout)
            out, obase, _, win = place(z, layout, fill=float("nan"))
            before = out.clone()
            if with_ce:
                ok(L.vqseg_dice_ce_sums_backward_f(base, sb, sc, sp, t_dev.data_ptr(), DICE_B, c, hw, IGNORE, gid.data_ptr(), gsd.data_ptr(),
                                                   gced.data_ptr(), obase, stream()))
            else:
                ok(L.vqseg_dice_sums_backward_f(base, sb, sc, sp, t_dev.data_ptr(), DICE_B, c, hw, IGNORE, gid.data_ptr(), gsd.data_ptr(),
                                                obase, stream()))
            torch.cuda.synchronize()
            got = unplace(out, layout, win).cpu()
            tag = f"C{c} HW{hw} {layout} g_ce {with_ce}"
            checked(got, ref, S, 1, F32, f"dice gradient {tag}", "dice backward")
            assert bool((got[ignored] == 0).all()), f"ignored pixels {tag}"
            if layout == "window":
                mask = torch.ones_like(out, dtype=torch.bool)
                mask[win] = False
                assert torch.equal(out.view(torch.int32)[mask], before.view(torch.int32)[mask]), f"bytes outside the window {tag}"


# ==================================================================================================================
# 3. vqseg_softmax_stats_f
# ==================================================================================================================
EPS32 = float(np.float32(1e-10))                               # the 1e-10f the kernel adds


@functools.lru_cache(maxsize=None)
def stats_inputs(c, hw):
    z = synth.uniform(8000 + 10 * c + hw, (2, c, hw), -6.0, 6.0)
    z[1, :, 0] = 2.5                                            # all logits equal: entropy log C, top 1 / C, label 0
    if hw > 16:
        z[:, :, 3] = 0.0
        z[:, 1, 3] = 115.0                                      # gap > 110: expf underflows to 0 for the other classes
        z[:, :, 5] = synth.uniform(5, (2, c), -1.0, 1.0)
        z[:, 0, 5] = -120.0                                     # one class underflows
        z[:, :, 7] = -3.0
        z[:, 0, 7] = z[:, 1, 7] = 5.0                           # exact tie of the first two
        z[:, :, 9] = -1.0
        z[:, c - 1, 9] = z[:, c - 2, 9] = 4.25                  # exact tie of the last two
        z[0, :, 11] = -0.75                                     # all equal
    return z


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("c", [2, 3, 4])
def test_softmax_stats(c, layout):
    """labels bit-exact against the first maximum.  q_c = p_c * inv carries rho_c roundings (softmax_rho); a = q + 1e-10f: 1, which moves
    logf's argument by u a, the logarithm by u: the ABSOLUTE term u q; logf 2; q * logf: 1; the C subtractions: C on sum |q log a|:
        |ent - ref| <= u sum_c [ q rho (|log a| + 1) + q + 3 q |log a| ] + C u sum_c q |log a|   (+ C 2^-126 (|log 1e-10| + 1): a probability
        in the subnormal range may be flushed)
    top = inv = 1 / sum: the sum's C - 1 additions and its terms' errors (their shares), the quotient: 1."""
    L = lib()
    for hw in (1, 255, 256, 257):
        z = stats_inputs(c, hw)
        zd = z.double()
        rho, q, share = softmax_rho(zd)
        a = q + EPS32
        la = torch.log(a).abs()
        ent_ref = -(q * torch.log(a)).sum(dim=1)
        ent_S = (q * rho * (la + 1) + q + 3 * q * la).sum(dim=1) + c * (q * la).sum(dim=1)
        top_ref = q.amax(dim=1)
        top_S = top_ref * (share[:, 0] + (c - 1) + 1)
        label_ref = torch.from_numpy(np.argmax(z.numpy(), axis=1))             # numpy: the first occurrence of the maximum
        assert abs(ent_ref[1, 0].item() - math.log(c)) < 1e-9 and top_ref[1, 0].item() == pytest.approx(1.0 / c, abs=1e-15)
        store, base, (sb, sc, sp), _ = place(z, layout)
        for drop in (None, 0, 1, 2):
            label, ent, top = nan_like((2, hw), torch.int64), nan_like((2, hw), F32), nan_like((2, hw), F32)
            args = [None if drop == i else o.data_ptr() for i, o in enumerate((label, ent, top))]
            ok(L.vqseg_softmax_stats_f(base, sb, sc, sp, 2, c, hw, *args, stream()))
            torch.cuda.synchronize()
            tag = f"C{c} HW{hw} {layout} without {drop}"
            if drop == 0:
                assert bool((label == -1).all()), tag
            else:
                assert torch.equal(label.cpu(), label_ref), f"labels {tag}"
            if drop == 1:
                assert bool(torch.isnan(ent).all()), tag
            else:
                checked(ent, ent_ref, ent_S, 1, F32, f"entropy {tag}", "softmax stats", extra=c * 2.0 ** -126 * (abs(math.log(EPS32)) + 1))
            if drop == 2:
                assert bool(torch.isnan(top).all()), tag
            else:
                checked(top, top_ref, top_S, 1, F32, f"top probability {tag}", "softmax stats")


# ==================================================================================================================
# 4. Prototype losses
# ==================================================================================================================
PROTO_CASES = [
    # variant, K, C, M, dtype, mask, gproto, (margin, scale, easy), branch
    (1, 3, 8, 255, F32, True, True, (0.0, 1.0, 1), "v1 without margin (use_margin = 0); keep mask; one short workgroup; KC = 24: G = 10, threads 240.. idle"),
    (1, 1, 24, 1, F32, False, False, (0.3, 8.0, 1), "K = 1, M = 1, keep == NULL; easy margin; (one class: the loss is ~1e-6, its bar an absolute 2e-6 -- gx carries the case)"),
    (1, 4, 40, 257, BF16, False, False, (1.5, 1.0, 0), "v1, non-easy margin on every class; bf16; a second workgroup of one row"),
    (1, 2, 64, 2 * 256 + 3, BF16, True, False, (0.5, 30.0, 0), "v1 at the golden's m05: exp(z) ~ 1e13; widest rows; three workgroups"),
    (1, 3, 64, 256, F32, True, True, (0.3, 8.0, 1), "v1 with a prototype gradient: KC = 192, G = 1, 64 idle threads in the fold"),
    (2, 1, 8, 256, F32, False, True, (0.0, 1.0, 1), "KC = 8: G = 32, no idle thread; conf == NULL; exactly one workgroup; (one class: loss ~1e-8, gx and gproto carry the case)"),
    (2, 2, 8, 2 * 256 + 3, F32, True, True, (1.5, 1.0, 0), "KC = 16: G = 16; three workgroups; conf with exact zeros"),
    (2, 2, 24, 257, F32, True, True, (0.3, 8.0, 1), "KC = 48: G = 5, threads 240.. idle (256 % 48 != 0)"),
    (2, 3, 24, 1, BF16, False, True, (0.0, 1.0, 1), "KC = 72: G = 3; M = 1: 255 dead rows in the tile"),
    (2, 3, 40, 2 * 256 + 3, BF16, True, True, (1.5, 1.0, 0), "KC = 120: G = 2; bf16 rows of 80 bytes"),
    (2, 4, 40, 256, BF16, True, False, (0.5, 30.0, 0), "v2 with gproto == NULL (no LDS tile); m05"),
    (2, 4, 64, 255, F32, False, True, (0.5, 30.0, 0), "KC = 256: G = 1, every thread one pair; m05; the largest LDS tile"),
]
PROTO_IDS = [f"v{v}-K{k}-C{c}-M{m}-{'bf16' if d == BF16 else 'f32'}" for v, k, c, m, d, *_ in PROTO_CASES]
G_LOSS = 3.0                                                   # the upstream factor


@functools.lru_cache(maxsize=None)
def proto_inputs(i):
    """fp32 CPU inputs of case i.  From M >= 255 on, rows 0..3 are: all zero (ordinary after the decoder's ReLU); 3 x its target
    prototype and -2 x its target prototype, both tilted to |cos| ~ 1 - 1e-3; a row of magnitude 1e-3."""
    variant, k, c, m, dtype, mask, _, _, _ = PROTO_CASES[i]
    seed = 9000 + 10 * i
    x = synth.uniform(seed, (m, c), -1.0, 1.0) * 2
    proto = F.normalize(synth.uniform(seed + 1, (k, c), -1.0, 1.0).double(), dim=1).float()
    labels = synth.labels(seed + 2, (m,), k)
    if m >= 255:
        p1, p2 = proto[labels[1]].double(), proto[labels[2]].double()
        v = synth.uniform(seed + 3, (2, c), -1.0, 1.0).double()
        tilt = math.sqrt(2e-3)                                  # cos = 1 / sqrt(1 + tilt^2) ~ 1 - 1e-3
        for row, p, s, vv in ((1, p1, 3.0, v[0]), (2, p2, -2.0, v[1])):
            vv = F.normalize(vv - (vv @ p) / (p @ p) * p, dim=0) * p.norm()
            x[row] = (s * (p + tilt * vv)).float()
        x[0] = 0.0
        x[3] *= 1e-3 / x[3].norm()
    w = None
    if mask and variant == 1:
        w = (synth.uniform(seed + 4, (m,)) >= 0.3).to(torch.uint8)             # ~30 % zeros
    elif mask:
        w = synth.uniform(seed + 4, (m,), -0.25, 1.0).clamp_min(0.0)           # [0, 1], ~20 % exact zeros
    if w is not None and m >= 255:
        w[0] = 1                                                # the all-zero row counts in every masked case
    return x, proto, labels, w


def proto_switch_rows(xd, proto, labels, variant, margin, easy):
    """rows a fp32 kernel may take through the other branch of phi_of: an fp64 cosine within 1e-5 of the switch (0: easy margin, th
    otherwise) -- the target's, and for variant 1 with a margin any class's (its margin goes on every class, weighted 1e-6).
    An all-zero row is not one of them: its cosine is 0 exactly, in fp32 as in fp64."""
    cos = F.normalize(xd, dim=1) @ proto.double().t()
    near = (cos - (0.0 if easy else math.cos(math.pi - margin))).abs() < 1e-5
    near = near.any(dim=1) if (variant == 1 and margin != 0) else near.gather(1, labels[:, None])[:, 0]
    return near & (xd != 0).any(dim=1)


def proto_switch_cap(i):
    """at most 1 % of a case's rows are left out of the per-row gradient check: a property of the seeds, checked on the CPU"""
    variant, k, c, m, dtype, _, _, (margin, scale, easy), _ = PROTO_CASES[i]
    x, proto, labels, _ = proto_inputs(i)
    out = proto_switch_rows(x.to(dtype).double(), proto, labels, variant, margin, easy)
    assert int(out.sum()) <= 0.01 * m, f"case {PROTO_IDS[i]}: {int(out.sum())} of {m} rows near the switch"
    return out


@pytest.mark.parametrize("i", range(len(PROTO_CASES)), ids=PROTO_IDS)
def test_proto_loss(i):
    """loss: 2e-6 relative (of max(1, |loss|), as test_loss_gpu.py; with K = 1 the softmax is constant, the loss ~0 and this an absolute
    2e-6 that says little: the two K = 1 rows are there for gx, gproto and the fold at G = 32).  gx per element: proto_gx_bound.  gproto: 2e-5 of the tensor scale.
    The all-zero row: finite, and g p_c / 1e-12 (F.normalize's clamp).  Rows past M untouched; the second call gives the same bits."""
    L = lib()
    variant, k, c, m, dtype, mask, want_gp, (margin, scale, easy), branch = PROTO_CASES[i]
    x, proto, labels, w = proto_inputs(i)
    skip = proto_switch_cap(i)
    xdev, xd = rnd(x, dtype)
    pd = proto.double()
    wd = torch.ones(m, dtype=torch.float64) if w is None else w.double()
    loss_ref, gx_ref, gp_ref = proto_ref(xd, pd, labels, wd, G_LOSS, variant, margin, scale, bool(easy))
    kk, S, extra, gx_closed = proto_gx_bound(xd, pd, labels, wd, G_LOSS, variant, margin, scale, bool(easy))
    p_dev, l_dev = proto.to(dev()), labels.to(dev())
    w_dev = None if w is None else w.to(dev())
    keep, conf = (ptr(w_dev), None) if variant == 1 else (None, ptr(w_dev))
    nbytes = L.vqseg_proto_loss_workspace_bytes(m, c, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    bf = int(dtype == BF16)
    loss = torch.full((), float("nan"), dtype=torch.float64, device=dev())
    ok(L.vqseg_proto_loss_forward_f(bf, xdev.data_ptr(), p_dev.data_ptr(), l_dev.data_ptr(), keep, conf, m, c, k, variant, scale, margin, easy,
                                    ws.data_ptr(), nbytes, loss.data_ptr(), stream()))
    torch.cuda.synchronize()
    err, bar = abs(loss.item() - loss_ref.item()), LOSS_BAR * max(1.0, abs(loss_ref.item()))
    note("prototype loss", f"loss {PROTO_IDS[i]}", err, bar)
    assert err <= bar, f"loss {loss.item()!r} ref {loss_ref.item()!r} ({branch})"
    g_dev = torch.tensor([G_LOSS], dtype=F32, device=dev())
    runs = []
    for _ in range(2):
        gx = nan_like((m + 1, c), dtype)                       # one sentinel row past M
        gp = nan_like((k, c), F32) if want_gp else None
        ok(L.vqseg_proto_loss_backward_f(bf, xdev.data_ptr(), p_dev.data_ptr(), l_dev.data_ptr(), keep, conf, m, c, k, variant, scale, margin,
                                         easy, g_dev.data_ptr(), gx.data_ptr(), ptr(gp), ws.data_ptr(), nbytes, stream()))
        torch.cuda.synchronize()
        runs.append((gx, gp))
    gx, gp = runs[0]
    assert bool(torch.isnan(gx[m]).all()), f"the row past M was written ({branch})"
    assert bool(torch.isfinite(gx[:m]).all())
    rows = ~skip
    checked(gx[:m].cpu()[rows], gx_ref[rows], S[rows], kk, dtype, f"gx {PROTO_IDS[i]} ({branch})", "prototype gx", extra=extra[rows])
    if m >= 255:                                                # the all-zero row: (sum_c gcos_c p_c) / 1e-12, which is what the closed form states
        assert bool((xd[0] == 0).all()) and not bool(skip[0])
        assert bool(((gx_ref[0] - gx_closed[0]).abs() <= 1e-9 * gx_ref[0].abs().max()).all())
        # (K = 1, variant 2: z = cos * phi(cos) has no slope at cos = 0 and there is no other class -- that row's gradient is 0)
        assert wd[0] == 1 and ((variant == 2 and k == 1) or gx_ref[0].abs().max() > 1e6 * G_LOSS / m), "the zero row is of the order g / (M 1e-12)"
    if want_gp:
        check_sum(gp, gp_ref, f"gproto {PROTO_IDS[i]} ({branch})")
        note("prototype gproto", PROTO_IDS[i], float((gp.double().cpu() - gp_ref).abs().max()), SUM_BAR * float(gp_ref.abs().max()))
        assert torch.equal(runs[1][1], gp), "gproto differs between two identical calls"
    assert torch.equal(runs[1][0][:m], gx[:m]), "gx differs between two identical calls"


# ==================================================================================================================
# 5. nnf.cps_loss_combine
# ==================================================================================================================
COMBINE_CASES = [
    # n_sup, n_cps, c, batch sizes, commitment vectors, levels, prototype scalars
    (1, 0, 2, (257,), 0, 0, 0),
    (2, 0, 3, (300, 1), 1, 1, 1),
    (0, 1, 4, (3,), 4, 3, 4),
    (2, 2, 3, (64, 257, 300, 1), 4, 1, 0),
    (1, 3, 4, (3, 300, 64, 257), 1, 3, 4),
]


@pytest.mark.parametrize("with_ce", [False, True], ids=["dice", "dice+ce"])
@pytest.mark.parametrize("n_sup,n_cps,c,bs,n_commit,levels,n_proto", COMBINE_CASES, ids=[f"{a}sup-{b}cps-c{c}" for a, b, c, *_ in COMBINE_CASES])
def test_cps_loss_combine(n_sup, n_cps, c, bs, n_commit, levels, n_proto, with_ce):
    """total and every stats entry: 2e-6 relative.  Gradients per element, k u |ref|, k from loss_combine_kernel and _CPSCombine.backward
    (which multiplies by the upstream factor: + 1):  g_inter = -w * (2 / den), w = weight / (float)n: den 1, the quotient 1, w 2, the
    product 1 -> 6;  g_sets = w * (num / (den * den)): den twice 2, the square 1, the quotient 1, w 2, the product 1 -> 8;
    g_ce[:, 0] = weight * ce_weight / t1: t1's cast 1, the product 1, the quotient 1 -> 4;  g_ce[:, 1] = -gce * (t0 / t1): gce's 3, the
    casts of t0 and t1 2, the quotient 1, the product 1 -> 8;  commitment: the product -> 2;  prototype (double, the weight a float in the kernel) -> 2."""
    from vq_seg_amd import nnf
    d = dev()
    f32 = lambda v: float(np.float32(v))                       # the floats the kernel receives
    cps_w, ce_w, com_w, pro_w, eps, up = 1.5, (0.5 if with_ce else 0.0), 0.25, 0.01, 1e-6, 1.25
    seed = 9500 + 10 * n_sup + n_cps

    def term(j, b):
        inter = synth.uniform(seed + 7 * j, (b, c), 0.0, 1000.0)
        sets = synth.uniform(seed + 7 * j + 1, (b, c), 1000.0, 4000.0)
        if not with_ce:
            return [inter, sets]
        ce = torch.stack([synth.uniform(seed + 7 * j + 2, (b,), 0.0, 5000.0), torch.floor(synth.uniform(seed + 7 * j + 3, (b,), 1000.0, 4000.0))], dim=1)
        return [inter, sets, ce]

    terms = [term(j, b) for j, b in enumerate(bs)]
    commits = [synth.uniform(seed + 100 + j, (levels,)) for j in range(n_commit)]
    protos = [synth.uniform(seed + 200 + j, ()).double() * 1.7 for j in range(n_proto)]
    # reference: float64 leaves of the same values, the weights as the floats the kernel gets
    rt = [[x.double().requires_grad_(True) for x in t] for t in terms]
    rc_ = [x.double().requires_grad_(True) for x in commits]
    rp = [x.clone().requires_grad_(True) for x in protos]
    total_ref, stats_ref = combine_ref(rt, n_sup, f32(cps_w), f32(ce_w), f32(eps), rc_, f32(com_w), rp, f32(pro_w))
    leaves_ref = [x for t in rt for x in t] + rc_ + rp
    g_ref = torch.autograd.grad(total_ref * up, leaves_ref, allow_unused=True)
    # the kernel (the wrapper allocates the gradient buffers itself: an entry it does not write is caught by the reference, not by a pre-fill)
    gt = [[x.to(d).requires_grad_(True) for x in t] for t in terms]
    gc = [x.to(d).requires_grad_(True) for x in commits]
    gp = [x.to(d).requires_grad_(True) for x in protos]
    got = nnf.cps_loss_combine(gt[:n_sup], gt[n_sup:], cps_w, ce_w, gc, com_w, gp, pro_w)
    assert got is not None
    total, stats = got
    leaves = [x for t in gt for x in t] + gc + gp
    g_got = torch.autograd.grad(total * up, leaves)
    tag = f"{n_sup} sup {n_cps} cps c {c} b {bs} ce {with_ce}"
    check_rel(total, total_ref.detach(), f"total {tag}", "loss combine")
    assert stats.shape == stats_ref.shape
    check_rel(stats, stats_ref.detach(), f"stats {tag}", "loss combine")
    ks = ([6, 8, (4, 8)] if with_ce else [6, 8]) * len(bs) + [2] * n_commit + [2] * n_proto
    for j, (a, r, k) in enumerate(zip(g_got, g_ref, ks)):
        assert a.shape == r.shape and bool(torch.isfinite(a).all()), (tag, j)
        if isinstance(k, tuple):
            checked(a[:, 0], r[:, 0], r[:, 0].abs(), k[0], F32, f"gradient of ce sums {tag}", "loss combine")
            checked(a[:, 1], r[:, 1], r[:, 1].abs(), k[1], F32, f"gradient of ce counts {tag}", "loss combine")
        else:
            checked(a, r, r.abs(), k, F32, f"gradient {j} {tag}", "loss combine")


# ==================================================================================================================
# 6. the nnf.dice_sums wrapper
# ==================================================================================================================
@pytest.mark.parametrize("arm", ["width-sliced view", "uint8 target", "ignore_index None"])
def test_dice_sums_wrapper(arm):
    """nnf.dice_sums / dice_ce_sums against the same fp64 reference: a width-sliced logits view (sh != w * sw: the copy path), a uint8
    target, ignore_index = None (the wrapper's 'none' value)."""
    from vq_seg_amd import nnf
    b, c, h, w = 2, 3, 9, 31
    full = synth.uniform(77, (b, c, h, w + 3), -8.0, 8.0)
    z = full[..., :w].contiguous()
    target = synth.labels(78, (b, h, w), c)
    ignore = None if arm == "ignore_index None" else IGNORE
    if ignore is not None:
        target[synth.uniform(79, (b, h, w)) < 0.2] = IGNORE
    x = (full.to(dev())[..., :w] if arm == "width-sliced view" else z.to(dev())).requires_grad_(True)
    assert x.is_contiguous() == (arm != "width-sliced view")
    t_dev = target.to(torch.uint8).to(dev()) if arm == "uint8 target" else target.to(dev())
    gi, gs, gce = synth.uniform(80, (b, c), -1.5, 1.5), synth.uniform(81, (b, c), -1.5, 1.5), synth.uniform(82, (b, 2), -1.5, 1.5)
    zd, tf = z.double().reshape(b, c, -1), target.reshape(b, -1)
    ign = NO_IGNORE if ignore is None else ignore
    ref = dice_pieces(zd, tf, ign)
    for with_ce in (False, True):
        out = nnf.dice_ce_sums(x, t_dev, ignore) if with_ce else nnf.dice_sums(x, t_dev, ignore)
        check_rel(out[0], ref[0], f"wrapper inter {arm}", "dice forward")         # 279 pixels an image: plain 2e-6, no floor
        check_rel(out[1], ref[1], f"wrapper sets {arm}", "dice forward")
        y = (out[0] * gi.to(dev())).sum() + (out[1] * gs.to(dev())).sum()
        g_ce = None
        if with_ce:
            check_rel(out[2][:, 0], ref[2][:, 0], f"wrapper ce {arm}", "dice forward")
            assert torch.equal(out[2][:, 1].cpu().double(), ref[2][:, 1])
            y = y + (out[2] * gce.to(dev())).sum()
            g_ce = gce[:, 0].double()
        (g,) = torch.autograd.grad(y, x)
        g_ref = dice_grad_ref(zd, tf, ign, gi.double(), gs.double(), g_ce)
        S = dice_grad_bound(zd, tf, ign, gi.double(), gs.double(), g_ce)
        checked(g.reshape(b, c, -1), g_ref, S, 1, F32, f"wrapper gradient {arm} ce {with_ce}", "dice backward")
