"""The fused supervised contrastive kernels (vqseg_supcon_*; nnf.supcon behind loss.SupConLoss) on the GPU, against a float64
restatement (tests/supcon_cases.py: restate64, dense (HW, HW) matrices) on the very float32 / bfloat16 values the kernel reads.

Pixel grids 5 x 7 (one ragged tile), 13 x 11, 16 x 16 (two row tiles, several column stages), 24 x 24 and 48 x 48 (column splits above 1:
the forward's partials of several workgroups per row are merged); C = 16 (half a gradient tile), 32, 64; both row types; targets at 1x and
2x the feature size; four label sets; feature scales 0.3, 1 and 3 (max z in the thousands: the reference's exp overflows); upstream
gradients 1 and 65536 (a gradient scaler's scale).

THE VALUE BAR, absolute on logA - logP (taken from loss * HW^2, which the kernel rounds to float32 once).  Let |x||y| be the largest
product of two row norms, zmax = max z >= 0 (post-ReLU rows), T the float32 temperature.
  * dot product:  float32 rows, v_mfma_f32_32x32x2_f32 = a chain of C fmaf's: |dot~ - dot| <= delta = C 2^-24 |x||y|;
                  bfloat16 rows, C / 16 v_mfma_f32_32x32x16_bf16, products exact, each instruction a sum of 17 addends aligned to the
                  largest one and truncated below 2^-24 of it (tools/micro/mfma_bf16_rounding.hip, the model of the VQ filter band):
                  delta = (C / 16) 17 2^-24 |x||y|.
  * t = dot * (log2 e / T) in float32: the constant's rounding, the product's and the subtraction of the running maximum: 3 * 2^-24 zmax.
  So every z carries at most eps_z = delta / T + 3 * 2^-24 zmax, and a log-sum-exp moves by at most the largest error of its arguments:
  2 eps_z for the difference of two.
  * v_exp_f32: 1 ulp, 2^-23 relative per term, the same on the sum; a lane's float32 partial sum holds at most HW / 2 + 2 terms (half a
    row's columns when the columns are not split, and the merge of the two halves): (HW / 2 + 2) 2^-24 relative; partials are merged in
    double; the result is rounded to float32 once: 2^-24 relative on the loss, so 2^-24 |logA - logP|.  A relative error r of a sum is
    an absolute r of its log; twice, for logA and logP.
  BAR = 2 (delta / T + 3 * 2^-24 zmax) + 2 (2^-23 + (HW / 2 + 2) 2^-24) + 2^-24 |logA - logP|.
Measured maxima per case: profiles/supcon.md.

THE GRADIENT BAR, relative L2 against float64 over the rows of both images.  g = g_all - g_pos is a difference of two parts that are each
evaluated to some relative accuracy; where the largest pair is a positive one the parts cancel (|g| down to 1e-5 of either part at
T = 0.04, and |g| = 0 exactly with a single class), and an error relative to |g| alone is then unbounded for ANY float32 evaluation of z
(the reference's own gradient is 2e-3 off float64 on such inputs: tests/supcon_cases.py).  So two things are asserted with one bar:
  (a) every case:            |g - g64| / (|g_all64| + |g_pos64|) <= GRAD_BAR   -- for the cancellation cases this is the absolute bound
                             |g - g64| <= GRAD_BAR (|g_all64| + |g_pos64|) on the error itself, with a right-hand side that float64 fixes
  (b) no cancellation, |g64| >= 0.3 |g_all64|:   |g - g64| / |g64| <= GRAD_BAR       (the plain relative L2)
GRAD_BAR is 4x the maximum of (b) measured on these 1440 cases (profiles/supcon.md; (a) never exceeds (b)'s maximum): float32 rows
4 * 2.1e-5 = 8.4e-5 (the worst case is scale 3, where the exponent of exp2(t - log2 A) is a float32 difference of numbers up to 2^13);
bfloat16 rows 4 * 3.43e-3 = 1.4e-2 (dz enters the second MFMA as bfloat16 and the gradient leaves as bfloat16: 2^-9 relative each, per
element), which is above the floor of bfloat16 output rounding, 2^-8 = 3.9e-3."""
import numpy as np
import pytest
import torch

from tests import supcon_cases as sc
from vq_seg_amd import nnf
from vq_seg_amd.loss import SupConLoss

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GRIDS = [(5, 7), (13, 11), (16, 16), (24, 24), (48, 48)]
CHANNELS = [16, 32, 64]
DTYPES = [torch.float32, torch.bfloat16]
SCALES = [0.3, 1.0, 3.0]
B = 3
GRAD_BAR = {torch.float32: 8.4e-5, torch.bfloat16: 1.4e-2}
assert GRAD_BAR[torch.bfloat16] >= 2.0 ** -8


def value_bar(ref, c, hw, dtype):
    t = float(np.float32(sc.TEMPERATURE))
    delta = (c * 2.0 ** -24 if dtype == torch.float32 else (c / 16) * 17 * 2.0 ** -24) * ref["norm"]
    diff = ref["diff"] if np.isfinite(ref["diff"]) else 0.0
    return 2 * (delta / t + 3 * 2.0 ** -24 * ref["zmax"]) + 2 * (2.0 ** -23 + (hw / 2 + 2) * 2.0 ** -24) + 2.0 ** -24 * abs(diff)


def case(grid, c, dtype, kind, scale, tmul):
    """-> the channels_last features on the GPU (values of `dtype`), the targets, and the float64 restatement for g = 1 (shared by the upstream gradients of a case)"""
    h, w = grid
    seed = 1000 + 97 * GRIDS.index(grid) + 13 * CHANNELS.index(c) + 5 * SCALES.index(scale) + 3 * sc.LABEL_KINDS.index(kind) + tmul
    x = sc.features(seed, (B, c, h, w), scale).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    target = sc.targets(seed + 7, B, h * tmul, w * tmul, kind).to(DEV)
    return x, target, sc.restate64(x, target)


def run(x, target, g):
    xg = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    loss = nnf.supcon(xg, target, sc.TEMPERATURE)
    (loss * g).backward()
    return loss.detach(), xg.grad


@pytest.mark.parametrize("kind", sc.LABEL_KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_value_and_gradient(grid, c, dtype, kind):
    hw = grid[0] * grid[1]
    failures = []
    for scale in SCALES:
        for tmul in (1, 2):
            x, target, ref = case(grid, c, dtype, kind, scale, tmul)
            assert nnf.supcon_supported(x, target)
            for g in (1.0, 65536.0):
                loss, grad = run(x, target, g)
                tag = f"supcon {grid[0]}x{grid[1]} C{c} {str(dtype)[6:]} {kind} scale {scale} target x{tmul} g {g:.0f}:"
                assert grad.dtype == dtype and grad.shape == x.shape
                assert float(grad[2:].float().abs().max()) == 0.0                    # images >= 2 do not enter
                assert bool(torch.isfinite(grad.float()).all()), tag
                bar = value_bar(ref, c, hw, dtype)
                if kind == "disjoint":                                                # no positive pair: +inf, as the reference
                    assert float(loss) == float("inf") and not ref["has"], tag
                    err = 0.0
                else:
                    err = abs(float(loss.double()) * float(hw) ** 2 - ref["diff"])
                got = torch.cat([sc.rows_of(grad, 0), sc.rows_of(grad, 1)])
                want = torch.cat([ref["g1"], ref["g2"]]) * g                          # disjoint: the logA part alone (restate64)
                part_all = torch.cat([ref["g1_all"], ref["g2_all"]]) * g
                n_err, n_want, n_all, n_pos = (float(v.norm()) for v in (got - want, want, part_all, part_all - want))
                rel_parts = n_err / (n_all + n_pos)
                rel_plain = n_err / n_want if n_want >= 0.3 * n_all else float("nan")
                print(f"{tag} zmax {ref['zmax']:.1f} diff {ref['diff']:.4g} value err {err:.3e} bar {bar:.3e} grad rel(parts) {rel_parts:.3e} "
                      f"rel(plain) {rel_plain:.3e}")
                if not err <= bar:
                    failures.append(f"{tag} |d (logA - logP)| = {err:.3e} > {bar:.3e}")
                if not rel_parts <= GRAD_BAR[dtype]:
                    failures.append(f"{tag} gradient rel L2 (parts) {rel_parts:.3e} > {GRAD_BAR[dtype]:.1e}")
                if rel_plain == rel_plain and not rel_plain <= GRAD_BAR[dtype]:
                    failures.append(f"{tag} gradient rel L2 {rel_plain:.3e} > {GRAD_BAR[dtype]:.1e}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_repeat_calls_are_bit_identical(dtype):
    x, target, _ = case((48, 48), 32, dtype, "three", 1.0, 1)                        # column splits above 1: partials of several workgroups
    (l0, g0), (l1, g1) = run(x, target, 1.0), run(x, target, 1.0)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    s0, s1 = nnf.supcon_stats(x, target, sc.TEMPERATURE), nnf.supcon_stats(x, target, sc.TEMPERATURE)
    assert torch.equal(s0, s1) and float(s0[0]) == float(l0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_layouts_and_the_module_agree(dtype):
    """an NCHW-contiguous tensor (copied into rows) and the module SupConLoss give the channels_last call's bits; (B, 1, Ht, Wt) labels too"""
    x, target, _ = case((13, 11), 32, dtype, "block255", 1.0, 2)
    l0, g0 = run(x, target, 1.0)
    l1, g1 = run(x.contiguous(), target.unsqueeze(1), 1.0)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    xg = x.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)
    l2 = SupConLoss(sc.TEMPERATURE)(xg, target)
    l2.backward()
    assert torch.equal(l0, l2.detach()) and torch.equal(g0, xg.grad)
    with pytest.raises(AssertionError, match="batch size is larger than 2"):
        SupConLoss()(x[:2], target[:2])


def test_other_shapes_take_the_torch_form():
    """C = 24 and float labels are outside the kernels: SupConLoss takes the torch-op form, on the GPU as well"""
    x = sc.features(1900, (B, 24, 6, 5), 0.5).to(DEV)
    target = sc.targets(1901, B, 6, 5, "three").to(DEV)
    assert not nnf.supcon_supported(x, target)
    ref = sc.restate64(x, target)
    assert abs(float(SupConLoss(sc.TEMPERATURE)(x, target).double()) * 900.0 - ref["diff"]) <= 1e-4
    x32 = sc.features(1902, (B, 32, 6, 5), 0.5).to(DEV)
    assert not nnf.supcon_supported(x32, target.float())
    a, b = SupConLoss(sc.TEMPERATURE)(x32, target.float()), SupConLoss(sc.TEMPERATURE)(x32, target)     # torch form / kernels
    assert abs(float(a) - float(b)) * 900.0 <= 1e-4


def test_memory_is_linear_in_hw():
    """96 x 96, C = 32: the dense (HW, HW) float32 matrix would be 340 MB; the call may add less than 16 MB"""
    h = w = 96
    x = sc.features(1950, (B, 32, h, w), 1.0).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    target = sc.targets(1951, B, h, w, "three").to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    loss = nnf.supcon(x, target, sc.TEMPERATURE)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(DEV) - base
    print(f"supcon 96x96 C32: peak memory rise {rise / 2 ** 20:.2f} MiB")
    assert rise < 16 * 2 ** 20
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())
