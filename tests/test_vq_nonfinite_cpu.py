"""The contract the GPU kernels are held to on non-finite and overflowing inputs (tests/test_vq_nonfinite_gpu.py) is the CPU chain
oracle's, oracle/vq_chain.c.  This module pins the oracle itself on those inputs against a plain NumPy restatement -- the same fmaf
chains, emulated exactly in float64, and the selection rule of its last loop: a NaN squared distance counts as 0
(`d > 0 ? d : 0`), the first minimum wins, a row whose distances are all +inf gets (0, +inf) -- and checks that the reference's op
sequence (oracle/torch_ref.py: torch.cdist -> argmin, vector_quantizer/vq_img.py:167-168) picks the same index."""
import warnings

import numpy as np
import pytest
import torch

from oracle import torch_ref, vq_chain
from tests import vq_poison as P

SHAPES = [(1029, 64, 256), (301, 20, 33)]


def fmaf32(a, b, c):
    """fmaf on float32 arrays, exactly: the product of two floats is exact in float64; the sum is rounded to odd in float64
    (TwoSum gives the rounding error), after which the rounding to float32 is the single correct one"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fin = np.isfinite(s) & np.isfinite(err) & (err != 0)
    si = s.view(np.int64).copy()
    even = fin & ((si & 1) == 0)
    # an inexact sum with an even last bit: move it one ulp towards the lost part, which makes it odd
    up = even & ((err > 0) == (s > 0))
    si[up] += 1
    si[even & ~up] -= 1
    return si.view(np.float64).astype(np.float32)


def chain_restated(rows, W):
    """order "mfma8" of oracle/vq_chain.c in NumPy: -> idx (N,), dmin (N,)"""
    x, w = rows.astype(np.float32), W.astype(np.float32)
    n, c = x.shape
    k = w.shape[0]
    cp = (c + 7) & ~7
    xp = np.zeros((n, cp), np.float32)
    xp[:, :c] = x
    wp = np.zeros((k, cp), np.float32)
    wp[:, :c] = w
    en = np.zeros(k, np.float32)
    for ch in range(c):
        en = fmaf32(w[:, ch], w[:, ch], en)
    lo, hi = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for ch in range(cp):
        if (ch & 7) < 4:
            lo = fmaf32(xp[:, ch], xp[:, ch], lo)
        else:
            hi = fmaf32(xp[:, ch], xp[:, ch], hi)
    xn = lo + hi
    acc = np.zeros((n, k), np.float32)
    for i in range(cp):
        j = i & 7
        ch = (i & ~7) + (4 if (j & 1) else 0) + (j >> 1)
        acc = fmaf32(np.broadcast_to(xp[:, ch:ch + 1], (n, k)), np.broadcast_to(wp[None, :, ch], (n, k)), acc)
    d = fmaf32(np.full((n, k), -2.0, np.float32), acc, np.broadcast_to(xn[:, None], (n, k)))
    d = d + en[None, :]
    d = np.where(d > 0, d, np.float32(0))                        # NaN and negatives -> 0
    d = np.sqrt(d)
    idx = np.empty(n, np.int64)
    dmin = np.empty(n, np.float32)
    for r in range(n):                                          # `if (d < best)` from best = +inf, bi = 0: the first minimum;
        j = int(np.argmin(d[r]))                                # np.argmin returns the first occurrence, and 0 for an all-inf row
        idx[r], dmin[r] = j, d[r, j]
    return idx, dmin, d


def check(rows, W, what, poisoned=None, expect_all_inf=False):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)         # the overflows and invalid operations are the point
        idx, dmin, d = chain_restated(rows.numpy(), W.numpy())
    ref_i, ref_d = vq_chain.assign(rows.numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
    k = W.shape[0]
    assert ref_i.min() >= 0 and ref_i.max() < k, what
    assert np.array_equal(ref_i, idx), f"{what}: {int((ref_i != idx).sum())} indices differ from the restatement"
    assert np.array_equal(ref_d.view(np.uint32), dmin.view(np.uint32)), f"{what}: distance bits differ from the restatement"
    assert not np.isnan(ref_d).any(), what
    all_inf = np.isinf(d).all(axis=1)
    assert (ref_i[all_inf] == 0).all() and np.isposinf(ref_d[all_inf]).all(), f"{what}: an all-inf row is not (0, +inf)"
    if expect_all_inf:
        assert all_inf[poisoned.numpy()].all(), f"{what}: the poison was meant to make every distance of its rows +inf"
    return ref_i, all_inf


def torch_argmin(rows, W):
    _, idx, _ = torch_ref.vq_lookup(rows, W)
    return idx.numpy()


@pytest.mark.parametrize("base", P.BASES)
@pytest.mark.parametrize("kind", P.ROW_POISONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_chain_oracle_on_poisoned_rows(shape, kind, base):
    n, c, k = shape
    rows0, W0 = P.base(base, n, c, k)
    rows, W, m = P.poison_rows(rows0, W0, kind)
    ref_i, all_inf = check(rows, W, f"{kind}/{base}", m, expect_all_inf=kind in ("norm_overflow", "dot_overflow"))
    # isolation on the oracle's side: the clean rows do not see the poisoned ones
    clean_i, _ = vq_chain.assign(rows0.numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
    assert np.array_equal(ref_i[~m.numpy()], clean_i[~m.numpy()])
    # the reference's op sequence picks the same code on the poisoned rows (the clean rows' near-ties are test_oracle_golden's matter)
    t_i = torch_argmin(rows, W)
    mp = m.numpy()
    assert np.array_equal(t_i[mp], ref_i[mp]), f"{kind}/{base}: torch.cdist -> argmin differs on {int((t_i[mp] != ref_i[mp]).sum())} poisoned rows"


@pytest.mark.parametrize("base", P.BASES)
@pytest.mark.parametrize("kind", P.CODE_POISONS)
def test_chain_oracle_on_poisoned_codebooks(kind, base):
    n, c, k = SHAPES[0]
    rows, W0 = P.base(base, n, c, k)
    W = P.poison_codebook(W0, kind)
    ref_i, _ = check(rows, W, f"{kind}/{base}")
    t_i = torch_argmin(rows, W)
    if kind == "huge_code":                                     # a code at distance +inf wins no row: every index is a clean near-tie matter
        assert (ref_i != P.POISONED_CODE).all()
        assert (t_i != P.POISONED_CODE).all()
    else:                                                       # rows that the non-finite code takes: the same rows on both sides
        assert np.array_equal(t_i == P.POISONED_CODE, ref_i == P.POISONED_CODE), f"{kind}/{base}"


def test_fmaf_emulation_is_single_rounding():
    """the restatement's fmaf against cases where rounding the float64 sum twice would differ"""
    a = np.array([1.0 + 2.0 ** -23, 3.0, 2.0 ** 100, np.inf, 1.0], np.float32)
    b = np.array([1.0 + 2.0 ** -23, 2.0 ** -24, 2.0 ** 100, 0.0, 2.0 ** -24], np.float32)
    c = np.array([2.0 ** -60, 1.0, 0.0, 1.0, 1.0 + 2.0 ** -23], np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = fmaf32(a, b, c)
    # (1 + 2^-23)^2 + 2^-60 = 1 + 2^-22 + 2^-46 + 2^-60: rounds to 1 + 2^-22;  3 * 2^-24 + 1 = 1 + 1.5 * 2^-23: above the half-way
    # point, rounds up to 1 + 2^-22;  2^200 overflows;  inf * 0 = NaN;  2^-24 + 1 + 2^-23 = 1 + 1.5 * 2^-23 exactly half-way between
    # 1 + 2^-23 and 1 + 2^-22: ties to even = 1 + 2^-22
    assert got[0] == np.float32(1.0 + 2.0 ** -22) and got[1] == np.float32(1.0 + 2.0 ** -22)
    assert np.isposinf(got[2]) and np.isnan(got[3]) and got[4] == np.float32(1.0 + 2.0 ** -22)
