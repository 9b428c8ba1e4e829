"""The acceptance bound of the dispatch-variant parity tests (tests/dispatch_cases.py: |y - ref| <= 2^-8 |ref| + K 2^-23 S,
elementwise) checked without a GPU: a correct kernel can meet it -- a plain fp32 matmul of the same operands, rounded to bf16,
does on every element -- and it has teeth: three ways a tiled kernel goes wrong each break it, where they should."""
import pytest
import torch

from tests import dispatch_cases as dc


@pytest.mark.parametrize("case", ["E1", "F2"])
def test_bound_admits_an_fp32_emulation_and_rejects_three_mutations(case):
    n, h, w, cin, cout, k, stride, pad, reflect = dc.CASES[case]
    x, wt = dc.operands(case)
    ref, S = dc.reference(case)
    K = dc.contraction(case)
    a = dc.patches(case, x.float())
    b = wt.reshape(cout, -1).t().contiguous()
    y = (a @ b).bfloat16()
    m = y.shape[0]
    assert y.shape == ref.shape == (m, cout) and m % 128 != 0                      # the last tile is ragged
    assert len(dc.violations(y, ref, S, K)) == 0
    # (1) one 64-channel K chunk dropped (a stage of the K loop skipped): wrong nearly everywhere
    a1 = a.clone()
    a1[:, 3 * 64:4 * 64] = 0
    bad = dc.violations((a1 @ b).bfloat16(), ref, S, K)
    assert len(bad) > 0.9 * m * cout
    # (2) the last M row replaced by its neighbour (a ragged tail clamped instead of masked): that row, and only it
    y2 = y.clone()
    y2[m - 1] = y[m - 2]
    bad = dc.violations(y2, ref, S, K)
    assert len(bad) > 0.9 * cout and bool((bad[:, 0] == m - 1).all())
    # (3) one output channel's weights shifted by one 64-channel chunk (a weight row fetched at the wrong offset): that channel
    co = cout - 3
    b3 = b.clone()
    b3[:, co] = torch.roll(b[:, co], 64)
    bad = dc.violations((a @ b3).bfloat16(), ref, S, K)
    assert len(bad) > 0.9 * m and bool((bad[:, 1] == co).all())
    # NaN left from the pre-fill is outside the bound too
    y4 = y.clone()
    y4[m // 2, 5] = float("nan")
    assert dc.violations(y4, ref, S, K).tolist() == [[m // 2, 5]]
