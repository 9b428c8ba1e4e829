"""The acceptance bounds of the stem and reflect-fold parity tests (tests/stem_cases.py) checked without a GPU: a correct kernel can
meet them -- an emulation with the kernels' arithmetic (fp32 matmuls of the bf16 operands; for split-3 three of them, an fp32 sum and a
re-split to hi + lo) does on every element -- and they have teeth: seven ways these kernels go wrong each break them, where they should."""
import pytest
import torch

from tests import stem_cases as sc
from tests import synth

EMULATED = [("S1", True), ("S2", True), ("S3", False)]


def _emulate(case, reflect, drop_tap=False, drop_lo_whi=False, right_off_by_one=False):
    """(acc fp32 [M, 64], acc3 fp32 [M, 64]): the bf16 launch's accumulator and the split-3 launch's, as the kernel forms them"""
    x, wt = sc.stem_operands(case)
    xh, xl = sc.split(x)
    wh, wl = sc.split(wt)
    ph = sc.stem_patches(xh, reflect, right_off_by_one)
    pl = sc.stem_patches(xl, reflect, right_off_by_one)
    bh, bl = sc.stem_weight_matrix(wh).contiguous(), sc.stem_weight_matrix(wl).contiguous()
    if drop_tap:                                                # (kh 6, kw 6, ci 2): the last of the 147 columns
        ph, pl = ph.clone(), pl.clone()
        ph[:, 146] = 0
        pl[:, 146] = 0
    hh = ph @ bh
    acc3 = hh + ph @ bl if drop_lo_whi else (hh + pl @ bh) + ph @ bl
    return hh, acc3


def _s3_out(acc3, scale, shift, relu=False, zero_lo=False):
    """v = hi + lo (float64) of [relu](acc * scale + shift) re-split as the epilogue does"""
    v = acc3 * scale + shift
    v = torch.relu(v) if relu else v
    hi, lo = sc.split(v)
    return hi.double() if zero_lo else hi.double() + lo.double()


@pytest.mark.parametrize("case,reflect", EMULATED, ids=[f"{c}-{'reflect' if r else 'zero'}" for c, r in EMULATED])
def test_stem_bounds_admit_an_fp32_emulation_and_reject_five_mutations(case, reflect):
    """The bounds of the raw, the affine and the split-3 check hold on every element of the emulation (printed: how much of each bound
    it uses), and the premise of the three-product scheme holds for these operands: |ref3 - true| <= 3 2^-18 S_true (the dropped
    x_lo w_lo and the second residuals of x and w; 2^-16 each in the worst case of a residual of half an ulp right above a power of
    two, a quarter of that and less on operands spread over the binade).

    The split-3 mutations are counted on the epilogue without ReLU, under the same bound: ReLU clips the half of the outputs whose
    pre-activation is negative (the scales have both signs) to an exact zero in kernel and reference alike, and a clipped element
    cannot show an error of any size -- the fractions below are of ALL elements."""
    n, h, w = sc.STEM_CASES[case]
    ho, wo = sc.stem_out_size(h, w)
    r = sc.stem_reference(case, reflect)
    scale, shift = sc.stem_affine()
    m = n * ho * wo
    total = m * sc.STEM_COUT
    acc, acc3 = _emulate(case, reflect)
    y = acc.bfloat16()
    assert y.shape == r["ref"].shape == (m, sc.STEM_COUT)
    raw_b = sc.stem_raw_bound(r)
    pre, aff_b = sc.stem_affine_bound(r, scale, shift)
    pre3, s3_b = sc.stem_s3_bound(r, scale, shift)
    want3 = pre3                                                # the mutations are judged without ReLU (see the docstring)
    v = _s3_out(acc3, scale, shift)
    print(f"{case}: raw uses {((y.double() - r['ref']).abs() / raw_b).max():.3f} of its bound, "
          f"split-3 {((v - want3).abs() / s3_b).max():.3f}, premise {((r['ref3'] - r['true']).abs() / (3 * 2.0 ** -18 * r['St'])).max():.3f}")
    assert len(sc.outside(y, r["ref"], raw_b)) == 0
    for relu in (False, True):
        ya = acc * scale + shift
        ya = (torch.relu(ya) if relu else ya).bfloat16()
        assert len(sc.outside(ya, torch.relu(pre) if relu else pre, aff_b)) == 0
    assert len(sc.outside(v, want3, s3_b)) == 0
    assert len(sc.outside(_s3_out(acc3, scale, shift, relu=True), torch.relu(pre3), s3_b)) == 0
    assert bool(((r["ref3"] - r["true"]).abs() <= 3 * 2.0 ** -18 * r["St"]).all())
    # the structure the GPU test asks of the output: hi the nearest bf16, lo a residual
    hi, lo = sc.split(torch.relu(acc3 * scale + shift))
    assert bool((lo.abs() <= 2.0 ** -8 * hi.abs()).all())

    # (1) the tap (kh 6, kw 6, ci 2) dropped (the last staged column, or the last K step's tail, skipped)
    a1, acc1 = _emulate(case, reflect, drop_tap=True)
    f1 = len(sc.outside(a1.bfloat16(), r["ref"], raw_b)) / total, len(sc.outside(_s3_out(acc1, scale, shift), want3, s3_b)) / total
    # (2) the lo w_hi product dropped: the image's low part never reaches the accumulator
    _y2, acc2 = _emulate(case, reflect, drop_lo_whi=True)
    f2 = len(sc.outside(_s3_out(acc2, scale, shift), want3, s3_b)) / total
    # (3) the output's lo plane zeroed
    f3 = len(sc.outside(_s3_out(acc3, scale, shift, zero_lo=True), want3, s3_b)) / total
    print(f"{case}: fraction outside: tap dropped {f1[0]:.2f} (raw) {f1[1]:.2f} (split-3), lo w_hi dropped {f2:.2f}, lo plane zeroed {f3:.2f}")
    assert min(f1) > 1 / 3 and f2 > 0.5 and f3 > 0.4
    # (4) the right-border reflection off by one (2W - 1 - iw): the output columns whose window crosses the right border, only them
    if reflect:
        a4, acc4 = _emulate(case, reflect, right_off_by_one=True)
        crossing = (w - 1 + 3 - 6 + 1) // 2                      # first ow with 2 ow - 3 + 6 >= w
        for bad in (sc.outside(a4.bfloat16(), r["ref"], raw_b), sc.outside(_s3_out(acc4, scale, shift), want3, s3_b)):
            assert len(bad) > 0 and bool((bad[:, 0] % wo >= crossing).all())
    # (5) output column 128 of every row replaced by column 127 (a strip seam clamped): that column, only it
    if wo > 128:
        rows = torch.arange(m)
        src = torch.where(rows % wo == 128, rows - 1, rows)
        for bad in (sc.outside(y[src], r["ref"], raw_b), sc.outside(v[src], want3, s3_b)):
            assert len(bad) > 0 and bool((bad[:, 0] % wo == 128).all())
    # NaN left from the pre-fill is outside every bound
    y6 = y.clone()
    y6[m // 2, 5] = float("nan")
    assert sc.outside(y6, r["ref"], raw_b).tolist() == [[m // 2, 5]]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_fold_bound_admits_an_fp32_emulation_and_finds_a_missing_corner(bf16):
    """(6) reflect_fold with the padded corner (0, 0) left out: exactly the pixels (1, 1) -- the only ones that corner reflects onto --
    violate, in every channel; a fold summed in fp32 in the kernel's order violates nowhere.  sum_bound is the bound that
    test_nn_kernels_gpu.check (which the GPU test calls) applies."""
    from tests.test_nn_kernels_gpu import BF16, F32, check
    dt = torch.bfloat16 if bf16 else torch.float32
    for case in sc.FOLD_CASES[1:4]:
        n, h, w, c = case
        gp, ref, S, t = sc.fold_reference(case, bf16)
        lim = sc.sum_bound(ref, S, t - 1, bf16)

        def emulate(skip_corner):
            acc = torch.zeros(n, h, w, c)
            g = gp.float()
            for i in range(h):
                for j in range(w):
                    rows = [i + 1] + ([0] if i == 1 else []) + ([h + 1] if i == h - 2 else [])
                    cols = [j + 1] + ([0] if j == 1 else []) + ([w + 1] if j == w - 2 else [])
                    for a in rows:
                        for b in cols:
                            if not (skip_corner and a == 0 and b == 0):
                                acc[:, i, j] += g[:, a, b]
            return acc.to(dt)

        good = emulate(False)
        assert len(sc.outside(good, ref, lim)) == 0
        check(good, ref, S, t - 1, BF16 if bf16 else F32, "fold emulation")
        one = t == 1
        assert bool(one.any()) and torch.equal(good[one], gp[:, 1:-1, 1:-1][one])
        bad = sc.outside(emulate(True), ref, lim)
        assert len(bad) == n * c and bool((bad[:, 1] == 1).all()) and bool((bad[:, 2] == 1).all())
        with pytest.raises(AssertionError):
            check(emulate(True), ref, S, t - 1, BF16 if bf16 else F32, "fold without its corner")


def test_ring_fold_bound_admits_an_fp32_emulation_and_finds_swapped_columns():
    """(7) the ring fold with the left and right column segments of the ring exchanged: violations exist and are confined to columns
    1 and w - 2 (the only pixels a column of the padded grid reflects onto)"""
    for n, h, w, c in ((2, 5, 7, 8), (1, 4, 4, 8), (1, 6, 5, 16)):
        ring = synth.uniform(61 + h, (n, sc.ring_len(h, w), c), -1, 1).bfloat16()
        g0 = synth.uniform(62 + w, (n, h, w, c), -1, 1).bfloat16()
        ref, S, k = sc.ring_fold_reference(g0, ring, h, w)
        assert int(k.max()) == 3 and int(k.min()) == 0
        lim = sc.sum_bound(ref, S, k, True)

        def emulate(swap):
            """gx + the ring positions, added one by one in fp32 (top / bottom row before the columns, as the kernel walks them)"""
            p = sc.ring_to_padded(ring.float(), h, w, swap_columns=swap)
            acc = g0.float().clone()
            for i in range(h):
                for j in range(w):
                    rows = [i + 1] + ([0] if i == 1 else []) + ([h + 1] if i == h - 2 else [])
                    cols = [j + 1] + ([0] if j == 1 else []) + ([w + 1] if j == w - 2 else [])
                    for a in rows:
                        for b in cols:
                            if (a, b) != (i + 1, j + 1):
                                acc[:, i, j] += p[:, a, b]
            return acc.bfloat16()

        good = emulate(False)
        assert len(sc.outside(good, ref, lim)) == 0
        assert torch.equal(good[k == 0], g0[k == 0])
        bad = sc.outside(emulate(True), ref, lim)
        assert len(bad) > 0 and bool(((bad[:, 2] == 1) | (bad[:, 2] == w - 2)).all())


def test_ring_order_round_trips_and_matches_the_documented_layout():
    n, h, w, c = 2, 4, 6, 3
    p = synth.uniform(70, (n, h + 2, w + 2, c), -1, 1)
    ring = sc.border_of(p)
    assert ring.shape == (n, sc.ring_len(h, w), c)
    assert torch.equal(ring[:, 3], p[:, 0, 3]) and torch.equal(ring[:, (w + 2) + 2], p[:, h + 1, 2])
    assert torch.equal(ring[:, 2 * (w + 2) + 1], p[:, 2, 0]) and torch.equal(ring[:, 2 * (w + 2) + h + 3], p[:, 4, w + 1])
    q = sc.ring_to_padded(ring, h, w)
    assert not q[:, 1:-1, 1:-1].any()
    q[:, 1:-1, 1:-1] = p[:, 1:-1, 1:-1]
    assert torch.equal(q, p)


def test_stem_weight_image_layout():
    """column kh * 24 + kw * 3 + ci holds bf16(w[co][ci][kh][kw]); the 3 pad columns of every kernel row and columns 168 .. 175 are zero"""
    _x, wt = sc.stem_operands("S1")
    img = sc.stem_weight_image(wt, False)
    img3 = sc.stem_weight_image(wt, True)
    assert img.shape == (64, 176) and img3.shape == (64, 2, 176) and img.dtype == img3.dtype == torch.bfloat16
    assert float(img[5, 4 * 24 + 2 * 3 + 1]) == float(wt[5, 1, 4, 2].bfloat16())
    assert not img.reshape(64, 176)[:, 168:].any() and not img[:, :168].reshape(64, 7, 24)[:, :, 21:].any()
    assert torch.equal(img3[:, 0], img)
    assert float(img3[9, 1, 6 * 24 + 6 * 3 + 2]) == float((wt[9, 2, 6, 6] - wt[9, 2, 6, 6].bfloat16().float()).bfloat16())
    assert int((img != 0).sum()) > 64 * 140
