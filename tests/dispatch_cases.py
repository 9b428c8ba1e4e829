"""Shapes, operands, fp64 references and the acceptance bound of the dispatch-variant parity tests
(tests/test_dispatch_variants_gpu.py; tests/test_dispatch_bound_cpu.py checks the bound itself without a GPU).

Every case convolves bf16-exact operands.  The reference is the same convolution in fp64 in unfold + matmul form, next to the
convolution S of |x| and |w| (the scale of the accumulation error).  Both are computed once per case and shared; nobody writes
into them."""
import functools

import torch
import torch.nn.functional as F

from tests import synth

# name -> n, h, w, cin, cout, k, stride, pad, reflect.  The smallest shapes that reach each instantiation by the dispatch rules of
# launch_conv_impl (conv_igemm.hip): the 256 x 128 tile needs Cout % 128 == 0, more than 8 64-channel K stages and
# ceil(M / 256) * ceil(Cout / 128) >= 512.
CASES = {
    "E1": (1, 89, 90, 576, 2048, 1, 1, 0, False),       # M = 8010: 32 M tiles (the last one 74 rows) x 16 chunks = 512
    "E2": (2, 85, 100, 576, 1024, 1, 1, 0, False),      # M = 17000: 67 tiles (67 % 8 = 3: five padding workgroups per chunk) x 8 chunks = 536
    "E3": (1, 253, 259, 64, 1024, 3, 2, 1, True),       # -> 127 x 130, M = 16510: 65 tiles x 8 chunks = 520; nine K stages
    "E4": (1, 179, 177, 576, 2048, 1, 2, 0, False),     # -> 90 x 89, M = 8010: 32 tiles x 16 chunks = 512
    "F1": (1, 9, 37, 1024, 256, 1, 1, 0, False),        # M = 333 (2 full 128-row tiles + 77 rows); 16 K stages
    "F2": (1, 9, 37, 2048, 512, 1, 1, 0, False),        # 32 K stages
    "F3": (1, 9, 37, 640, 192, 1, 1, 0, False),         # the second 128-wide chunk holds 64 channels
    "F4": (1, 9, 37, 128, 32, 1, 1, 0, False),
    "F5": (1, 9, 37, 128, 64, 1, 1, 0, False),
}


def out_size(case):
    n, h, w, cin, cout, k, stride, pad, reflect = CASES[case]
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def _seed(case):
    return 1000 + 17 * sorted(CASES).index(case)


@functools.lru_cache(maxsize=None)
def operands(case):
    """x [n, h, w, cin] bf16, w [cout, cin, k, k] fp32 holding bf16 values (what vqseg_conv_pack_weights_f32 rounds to)"""
    n, h, w, cin, cout, k, stride, pad, reflect = CASES[case]
    x = synth.uniform(_seed(case), (n, h, w, cin), -1, 1).bfloat16()
    wt = (synth.uniform(_seed(case) + 1, (cout, cin, k, k), -1, 1) * (2.0 / (cin * k * k)) ** 0.5).bfloat16().float()
    return x, wt


def patches(case, x):
    """the im2col matrix [M, cin * k * k] of x (any float dtype; columns ordered (ci, kh, kw) as w.reshape(cout, -1))"""
    n, h, w, cin, cout, k, stride, pad, reflect = CASES[case]
    if k == 1:
        return x[:, ::stride, ::stride, :].reshape(-1, cin)
    xp = F.pad(x.permute(0, 3, 1, 2), (pad, pad, pad, pad), mode="reflect" if reflect else "constant")
    return F.unfold(xp, k, stride=stride).transpose(1, 2).reshape(-1, cin * k * k)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(ref, S): the fp64 convolution [M, cout] of the case's operands, and the same convolution of |x| and |w|"""
    x, wt = operands(case)
    a = patches(case, x.double())
    b = wt.double().reshape(wt.shape[0], -1).t()
    return a @ b, a.abs() @ b.abs()


def contraction(case):
    n, h, w, cin, cout, k, stride, pad, reflect = CASES[case]
    return k * k * cin


def bound(ref, S, K):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 S, elementwise.  Products of two bf16 values are exact in fp32; an fp32 accumulation of K of
    them in any order errs by at most K u S, with u = 2^-23 so that an adder that truncates inside the MFMA is covered; the final
    rounding to bf16 is within 2^-8 relative (one ulp).  No term comes from the code under test."""
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * S


def violations(y, ref, S, K):
    """coordinates (row, channel) of the elements of y outside the bound (NaN counts as outside)"""
    return (~((y.double() - ref).abs() <= bound(ref, S, K))).nonzero()
