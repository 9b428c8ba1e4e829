"""Non-finite and overflowing inputs of the VQ assignment, shared by tests/test_vq_nonfinite_cpu.py (the oracle's contract) and
tests/test_vq_nonfinite_gpu.py (the kernels against that contract).  Not a test module.

Contract (oracle/vq_chain.c, the selection loop after the dot products; it is what the reference's cdist -> argmin returns):
a NaN squared distance counts as 0, the lowest code attaining the minimum wins, a row whose distances are all +inf gets code 0
and distance +inf.  Every row, whatever it holds, has a code in [0, K) and defined distance bits."""
import numpy as np
import torch

from tests import synth

ROW_POISONS = ["nan_one", "nan_all", "pos_inf", "neg_inf", "inf_both", "norm_overflow", "dot_overflow", "dot_overflow_2p28"]
CODE_POISONS = ["nan_code", "inf_code", "huge_code"]
BASES = ["relu", "signed"]
POISONED_CODE = 5


def base(kind, n, c, k, seed=300):
    """clean rows (n, c) and codebook (k, c), fp32: post-ReLU rows against a sparse codebook, or both uniform in (-2, 2) (signed and
    dense: what makes a -Inf entry give +inf to EVERY code of a row)"""
    if kind == "relu":
        return synth.relu_features(seed, (n, c)), synth.relu_features(seed + 1, (k, c), sparsity=0.3, scale=1.5)
    return synth.uniform(seed + 3, (n, c), -2, 2), synth.uniform(seed + 4, (k, c), -2, 2)


def poisoned_mask(n):
    """the same rows for every kind: every 7th (every wave and every 128-row tile mixes clean and poisoned rows), rows 256 .. 511
    (a whole 256-row workgroup of the resolve stage; clipped at n), row 0 and the last row (the resolve stage re-reads row N - 1
    for the lanes past the end)"""
    m = torch.zeros(n, dtype=torch.bool)
    m[::7] = True
    m[256:512] = True
    m[0] = True
    m[n - 1] = True
    return m


def poison_rows(rows, W, kind):
    """-> (poisoned rows, codebook, mask of the poisoned rows).  Every poison value is a NaN, an Inf or a power of two: exact in
    fp32 and in bf16.  The codebook changes only for the dot_overflow kinds (scaled by a power of two: the clean rows' call uses
    the same scaled codebook)."""
    n, c = rows.shape
    rows, W = rows.clone(), W.clone()
    m = poisoned_mask(n)
    r = torch.nonzero(m)[:, 0]
    col = (r * 5 + 3) % c                                       # the poisoned channel moves with the row
    col2 = (col + 1 + r % (c - 1)) % c                          # a second, different channel
    nan, inf = float("nan"), float("inf")
    if kind == "nan_one":
        rows[r, col] = nan
    elif kind == "nan_all":
        rows[r] = nan
    elif kind == "pos_inf":
        rows[r, col] = inf
    elif kind == "neg_inf":
        rows[r, col] = -inf
    elif kind == "inf_both":
        rows[r, col] = inf
        rows[r, col2] = -inf
    elif kind == "norm_overflow":                               # |x|^2 = 2^140 = +inf in fp32, x . e ~ 2^71 stays finite
        rows[r, col] = 2.0 ** 70
        rows[r, col2] = 2.0 ** 70
    elif kind == "dot_overflow":                                # as specified: 2^100 rows, codebook x 2^20.  |x|^2 overflows; the dot
        rows[r] = 2.0 ** 100                                    # products reach ~2^125 (C = 64) and do NOT overflow (fp32 max 2^128) ...
        W = W * 2.0 ** 20
    elif kind == "dot_overflow_2p28":                           # ... so the same with the codebook x 2^28: single products overflow
        rows[r] = 2.0 ** 100
        W = W * 2.0 ** 28
    else:
        raise ValueError(kind)
    return rows, W, m


def poison_codebook(W, kind):
    W = W.clone()
    if kind == "nan_code":
        W[POISONED_CODE, 7] = float("nan")
    elif kind == "inf_code":
        W[POISONED_CODE, 7] = float("inf")
    elif kind == "huge_code":                                   # |e|^2 overflows, the entries stay finite
        W[POISONED_CODE] = W[POISONED_CODE] * 2.0 ** 70
    else:
        raise ValueError(kind)
    return W


def bits(t):
    """bit patterns of a tensor / array as integers, so that NaNs compare (and their payloads)"""
    a = t.detach().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    a = a.contiguous()
    if a.dtype == torch.bfloat16:
        return a.view(torch.int16).numpy()
    if a.dtype == torch.float32:
        return a.view(torch.int32).numpy()
    return a.numpy()
