"""The acceptance bound of the precise-convolution parity tests (tests/precise_cases.py: |y - ref| <= 2^-16 S + 3 K 2^-23 S +
2^-23 |ref|, elementwise) checked without a GPU: the documented arithmetic of the kernels -- round-to-nearest-even split of both
operands, three products, fp32 accumulation -- emulated in torch meets it on every case, and it has teeth: five ways a tiled split
kernel goes wrong each break it, where they should.  `pytest -s` prints the worst error / bound of every case and mutation."""
import pytest
import torch

from tests import precise_cases as pc


def _check(case, mutation=None):
    ref, S = pc.reference(case)
    y = pc.emulate(case, mutation)
    K, prev = pc.contraction(case), pc.prev_rows(case)
    bad = pc.violations(y, ref, S, K, prev)
    print(f"{case} {mutation or 'faithful'}: worst error / bound {pc.worst(y, ref, S, K, prev):.3g}, {len(bad)} of {ref.numel()} outside")
    return bad, ref.shape


@pytest.mark.parametrize("case", pc.PRECISE)
def test_emulated_split_arithmetic_is_inside_the_bound_and_five_mutations_are_not(case):
    bad, (rows, cols) = _check(case)
    assert len(bad) == 0, f"first (row, column) outside: {bad[0].tolist()}"
    # m1: one cross product dropped everywhere
    bad, _ = _check(case, "m1")
    assert len(bad) > 0
    # m2 / m3: ... on one K stage / the second concat source's lo image: wherever the split term dominates the bound
    if pc.sharp(case):
        assert len(_check(case, "m2")[0]) > 0
        if pc.second_source(case) is not None:
            assert len(_check(case, "m3")[0]) > 0
    # m4: the last row, and only it
    bad, _ = _check(case, "m4")
    assert len(bad) > 0 and bool((bad[:, 0] == rows - 1).all())
    # m5: that column, and only it
    bad, _ = _check(case, "m5")
    assert len(bad) > 0 and bool((bad[:, 1] == cols + pc.M5_COLUMN).all())
    # a NaN left from the pre-fill is outside the bound too
    ref, S = pc.reference(case)
    y = pc.emulate(case)
    y[rows // 2, 5] = float("nan")
    assert pc.violations(y, ref, S, pc.contraction(case), pc.prev_rows(case)).tolist() == [[rows // 2, 5]]


@pytest.mark.parametrize("case", [c for c in pc.CASES if pc.kind(c) != "fwd"])
def test_gemm_form_of_the_gradients_is_autograd_s_gradient(case):
    """the unfold + matmul references of the data and weight gradients against autograd in fp64 on the explicitly padded input"""
    ref, S = pc.reference(case)
    want = pc.autograd_reference(case)
    assert want.shape == ref.shape
    assert bool(((ref - want).abs() <= 1e-13 * S).all())


def test_operands_have_full_mantissas_zeros_and_bf16_exact_values_and_no_lo_underflows():
    for case in pc.PRECISE:
        for v in pc.operands(case)[:2]:
            nz = v[v != 0]
            assert float(nz.abs().min()) >= 2.0 ** -20 and float(nz.abs().max()) <= 4.0
            assert bool((v < 0).any()) and bool((v > 0).any())
            hi, lo = pc.split(v)
            exact = (hi == v)
            assert 0.005 < float((v == 0).float().mean()) < 0.08
            assert 0.05 < float((exact & (v != 0)).float().mean()) < 0.25
            assert bool(((lo != 0) | exact).all())                                    # no lo part flushed to zero
            assert bool(((v - hi).abs() <= 2.0 ** -8 * v.abs()).all())                # the figures of the bound's derivation
            assert bool(((v - hi - lo).abs() <= 2.0 ** -17 * v.abs()).all())
            assert bool(((v - hi - lo).abs() > 2.0 ** -18 * v.abs()).any())           # ... and 2^-18 would not hold
            assert bool((v.view(torch.int32) & 0xFF != 0).float().mean() > 0.8)       # low mantissa bits in use
    for case in pc.FAST:
        for v in pc.operands(case)[:2]:
            assert torch.equal(v.bfloat16().float(), v)


def test_every_claimed_instantiation_has_a_case_and_every_precise_one_a_sharp_case():
    """ids as conv_internal.h builds them: conv_variant_igemm(bn, precise, 32, false), conv_variant_wgrad_tap(tm, tn, precise)"""
    igemm = {0x2000100 | (bn // 32) << 16 | p << 4 for bn in (128, 64, 32) for p in (0, 1)}
    wgrad = {0x6000000 | tm << 16 | tn << 12 | p << 4 for tm in (4, 2, 1) for tn in (4, 1) for p in (0, 1)}
    assert set(pc.VARIANTS) == igemm | wgrad and len(igemm) == 6 and len(wgrad) == 12
    assert sorted(c for cs in pc.VARIANTS.values() for c in cs) == sorted(pc.CASES)
    for vid, cases in pc.VARIANTS.items():
        precise = bool(vid & 0x10)
        assert all(pc.fast(c) != precise for c in cases)
        if precise:
            assert any(pc.sharp(c) for c in cases), hex(vid)
        for c in cases:                                                              # the dispatch rules of launch_conv_impl / launch_wgrad_impl
            knd, n, h, w, c1, c2, cout, k, stride, pad, reflect, acc = pc.CASES[c]
            cin = c1 + c2
            if knd == "wgrad":
                tm, tn = (4 if cout >= 128 else 2 if cout >= 64 else 1), (4 if cin % 128 == 0 else 1)
                assert vid == 0x6000000 | tm << 16 | tn << 12 | precise << 4, c
            else:
                launched_cout = cin if knd == "dgrad" else cout
                bn = 128 if launched_cout >= 128 else 64 if launched_cout >= 64 else 32
                assert vid == 0x2000100 | (bn // 32) << 16 | precise << 4, c
                assert pc.reference(c)[0].shape[0] % 128 != 0, c                    # the last pixel tile is ragged
    # at least one case runs three or more K stages per tap
    assert any(len(pc.stages(c)) >= 3 * pc.CASES[c][7] ** 2 for c in pc.PRECISE if pc.kind(c) != "wgrad")
