"""The acceptance bound of the bf16 convolution parity tests (tests/fast_cases.py: dispatch_cases.bound, |y - ref| <= 2^-8 |ref| +
K 2^-23 S elementwise, and what fold_reference / the affine epilogues derive from it) checked without a GPU on one patch case, one
stride-2 data gradient and one merged-fold reflect case: the documented arithmetic -- an fp32 matmul of the same bf16 operands,
round to nearest bf16; fold: parts rounded, summed in fp32, rounded once; affine epilogue: two roundings -- is inside on every
element, and five ways a tiled bf16 kernel goes wrong are outside, where they should be.  A store that truncates instead of
rounding passes the 2^-7 max-norm bar the kernels were held to before and fails this one.  `pytest -s` prints every figure.

The sixth mutation one could think of for the fold -- the ring value added to the body's fp32 accumulator BEFORE the body is rounded,
one bf16 rounding fewer than reflect_s2_ring_add_kernel documents -- is not here: it is closer to the fp64 reference than the
documented arithmetic, and an upper bound on the error of three roundings cannot reject two.  The bound is not tightened to fit it;
bit-identity of the two paths away from row 1 / column 1 (tests/test_optim_gpu.py) is what pins the order of operations."""
import pytest
import torch

from tests import dispatch_cases as dc
from tests import fast_cases as fc

PATCH_CASE, S2_CASE, FOLD_CASE = "P1", "S3", "R1"


def _want_and_limit(case):
    if fc.kind(case) == "fold":
        return fc.fold_reference(case)
    return fc.reference(case)[0], fc.limit(case)


def _check(case, mutation=None):
    """-> (coordinates outside the bound, shape); prints the worst error / bound"""
    want, limit = _want_and_limit(case)
    y = fc.emulate(case, mutation).double()
    err = (y - want).abs()
    pos = limit > 0
    bad = (~(err <= limit)).nonzero()
    print(f"{case} {mutation or 'faithful'}: worst error / bound {float((err[pos] / limit[pos]).max()):.3g}, {len(bad)} of {want.numel()} outside")
    return bad, want.shape


@pytest.mark.parametrize("case", [PATCH_CASE, S2_CASE, FOLD_CASE])
def test_emulated_bf16_arithmetic_is_inside_the_bound_and_the_mutations_are_not(case):
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    bad, (rows, cols) = _check(case)
    assert len(bad) == 0, f"first (row, column) outside: {bad[0].tolist()}"
    # 1. a truncating store
    assert len(_check(case, "truncate")[0]) > 0
    # 2. one chunk of one tap dropped
    assert len(_check(case, "chunk")[0]) > 0
    # 4. the last row, and only it
    bad, _ = _check(case, "row")
    assert len(bad) > 0 and bool((bad[:, 0] == rows - 1).all())
    # a NaN left from the pre-fill is outside the bound; an element whose bound is 0 must be exactly 0
    want, limit = _want_and_limit(case)
    y = fc.emulate(case).double()
    y[rows // 2, 5] = float("nan")
    assert (~((y - want).abs() <= limit)).nonzero().tolist() == [[rows // 2, 5]]
    if knd == "dgrad" and stride == 2:
        zero = (limit == 0)
        assert bool(zero.any()) and bool((fc.emulate(case)[zero] == 0).all())       # even sizes: the padded grid's last row and column, S = 0


def test_a_truncating_store_passes_the_max_norm_bar_and_fails_the_elementwise_bound():
    """what the new bar adds: on the patch case's operands truncation is within 2^-7 of the largest element (the bar of
    test_nn_gpu._patch_case) -- and outside dispatch_cases.bound on thousands of elements"""
    ref, S = fc.reference(PATCH_CASE)
    y = fc.emulate(PATCH_CASE, "truncate").double()
    max_norm = float((y - ref).abs().max() / ref.abs().max())
    outside = dc.violations(y, ref, S, fc.contraction(PATCH_CASE))
    print(f"{PATCH_CASE} truncate: max-norm error {max_norm:.4g} (bar {2 ** -7:.4g}), {len(outside)} of {ref.numel()} outside the elementwise bound")
    assert max_norm < 2 ** -7
    assert len(outside) > ref.numel() // 100
    faithful = fc.emulate(PATCH_CASE).double()
    assert float((faithful - ref).abs().max() / ref.abs().max()) < 2 ** -7 and len(dc.violations(faithful, ref, S, fc.contraction(PATCH_CASE))) == 0


def test_a_zero_halo_column_is_seen_at_the_tile_edge_and_only_there():
    """3. tap (1, 0) reads zero for the pixels in column TILE_W: only those pixels leave the bound"""
    knd, n, h, w, *_rest = fc.geometry(PATCH_CASE)
    bad, _ = _check(PATCH_CASE, "halo")
    assert len(bad) > 0 and bool((bad[:, 0] % w == fc.TILE_W).all())
    assert len(set((bad[:, 0] // w).tolist())) == n * h                              # every image row's edge pixel


def test_a_fold_without_the_padded_corner_is_seen_at_pixel_1_1_and_only_there():
    """5. x (1, 1) sums four padded positions; without the corner it is outside, everything else inside"""
    knd, n, h, w, *_rest = fc.geometry(FOLD_CASE)
    bad, _ = _check(FOLD_CASE, "corner")
    assert len(bad) > 0 and bool((bad[:, 0] % (h * w) == w + 1).all())
    assert len(set((bad[:, 0] // (h * w)).tolist())) == n


def test_fold_bound_is_the_plain_bound_where_the_ring_kernel_adds_nothing():
    """pixels off row 1 / column 1 keep dispatch_cases.bound of their own padded position; on them the bound is larger"""
    knd, n, h, w, c1, *_rest = fc.geometry(FOLD_CASE)
    _want, lim = fc.fold_reference(FOLD_CASE)
    plain = fc.limit(FOLD_CASE).reshape(n, h + 2, w + 2, c1)[:, 1:-1, 1:-1]
    t = fc.touched(FOLD_CASE)
    lim = lim.reshape(n, h, w, c1)
    assert torch.equal(lim[:, ~t], plain[:, ~t]) and bool((lim[:, t] > plain[:, t]).all())


@pytest.mark.parametrize("form", ["affine", "bits"])
def test_emulated_affine_epilogue_with_two_roundings_is_inside_its_bound(form):
    """t = bf16(fma(acc, scale, shift)), y = bf16([relu](t + addend)): inside 2^-8 |y_ref| + 2^-8 |t_ref| + K 2^-23 S |scale|
    (test_256x128_tile_fused_affine_epilogues_on_the_pair_grid's derivation); with both roundings truncating it is not"""
    case = PATCH_CASE
    ref, S = fc.reference(case)
    scale, shift, res, keep = fc.epilogue_operands(case)
    y_ref, limit = fc.epilogue_reference(case, form)
    acc = torch.matmul(*fc.gemm(case))
    for rnd, inside in ((fc.round_bf16, True), (fc.truncate_bf16, False)):
        t = rnd(acc * scale + shift)
        y = rnd(torch.relu(t + res)) if form == "affine" else rnd(t + torch.where(keep, res, torch.zeros(())))
        err = (y.double() - y_ref).abs()
        bad = int((~(err <= limit)).sum())
        print(f"{case} {form} {'rounded' if inside else 'truncated'}: worst error / bound {float((err / limit).max()):.3g}, {bad} outside")
        assert (bad == 0) == inside


def test_every_listed_instantiation_has_a_case_and_every_case_a_test_family():
    """the ids of the issue's section A, the three CLS ids and the tap / stride cases of C are in VARIANTS; every case belongs to exactly
    one instantiation and to at least one of the lists tests/test_fast_conv_gpu.py parametrises over; the id of every case follows
    from its geometry and options by the dispatch rules of launch_conv3x3_patch / launch_conv_impl / launch_dgrad_s2_fold"""
    assert set(fc.A_IDS) <= set(fc.VARIANTS) and set(fc.CLS_IDS) <= set(fc.VARIANTS)
    assert all(len(cs) > 0 for cs in fc.VARIANTS.values())
    assert sorted(c for cs in fc.VARIANTS.values() for c in cs) == sorted(fc.CASES)
    families = fc.A_CASES + fc.EPILOGUE_CASES + ["G1"] + fc.C_CASES + fc.S2_K3_CASES + fc.S2_K1_CASES + fc.FOLD_CASES
    assert set(families) == set(fc.CASES)
    assert not any(vid & 8 for vid in fc.VARIANTS)                                   # no split-3 instantiation: out of scope
    assert {fc.variant_of(c) for c in fc.A_CASES} == set(fc.A_IDS)
    assert {fc.variant_of(c) for c in fc.FOLD_CASES} == set(fc.CLS_IDS)
    for c in fc.CASES:
        assert fc.variant_of(c) == _dispatch(c), c
    # several Cout chunks (the XCD-pair launch of the patch tests) on the tap ring, the chunk stages and the 32-channel tap ring
    multi = [c for c in fc.A_CASES if fc.geometry(c)[6] > 32 * (fc.variant_of(c) >> 16 & 15)]
    assert {fc.variant_of(c) for c in multi} >= {0x3143210, 0x3140110, 0x3143110}
    # C: 3x3 stride 1 on ragged sizes, 3x3 stride 2 with zero and reflect padding, 1x1 stride 2, a concat on a 64-channel boundary
    geo = [fc.geometry(c) for c in fc.C_CASES]
    assert {(g[7], g[8]) for g in geo} == {(3, 1), (3, 2), (1, 2)}
    assert {g[10] for g in geo if g[7:9] == (3, 2)} == {True, False} and any(g[5] == 64 and g[4] % 64 == 0 for g in geo)
    assert all(fc.reference(c)[0].shape[0] % 128 != 0 for c in fc.C_CASES + fc.S2_K3_CASES + fc.S2_K1_CASES)
    assert all(fc.operands(c)[i].bfloat16().float().equal(fc.operands(c)[i]) for c in fc.CASES for i in (0, 1))


def _dispatch(case):
    """the id by the rules read from the launchers, at the options of the case (defaults: conv_internal.h's ConvOptions)"""
    knd, n, h, w, c1, c2, cout, k, stride, pad, reflect = fc.geometry(case)
    opt = {"conv3x3_patch_min_workgroups": 128, "conv3x3_patch_tile512_min_workgroups": 512, "conv3x3_patch_unroll": 1,
           "conv3x3_patch_chunk_stage": 1, **fc.options(case)}
    if knd == "fold":
        if c1 < 128:
            return fc.glds_id(64, 3, 1, cls=True)
        return fc.glds_id(128, 1, 4, cls=True) if 4 * (cout // 64) <= 8 else fc.glds_id(128, 2, 1, cls=True)
    if knd == "dgrad":                                          # launched: gy's channels in, the layer's input channels out
        l_cin, l_c1, l_cout = cout, cout, c1 + c2
        taps = 1 if stride == 2 else k * k                      # stride 2: the last parity class has one tap
        patch_shape = stride == 1
        ho, wo = h, w
    else:
        l_cin, l_c1, l_cout, taps = c1 + c2, c1, cout, k * k
        patch_shape = k == 3 and stride == 1
        ho, wo = fc.out_size(case)
    k64 = l_cin % 64 == 0 and (l_c1 == l_cin or l_c1 % 64 == 0)
    bn = 128 if l_cout >= 128 else 64 if l_cout >= 64 else 32
    tw = 32 if w % 32 == 0 else 16
    if patch_shape and w % tw == 0 and h % (256 // tw) == 0 and (l_cout % 128 == 0 or l_cout in (32, 64)) and l_cin % 32 == 0 and l_c1 % 32 == 0:
        pbn = 128 if l_cout % 128 == 0 else l_cout
        tiles = n * (h // (256 // tw)) * (w // tw)
        if tiles * (l_cout // pbn) >= opt["conv3x3_patch_min_workgroups"]:
            if (l_cout == 32 or (l_cout == 64 and l_cin >= 64)) and h % (512 // tw) == 0 and \
                    n * (h // (512 // tw)) * (w // tw) >= opt["conv3x3_patch_tile512_min_workgroups"]:
                return fc.patch_id(l_cout, 0, True, 32, 512)
            if not k64:
                if opt["conv3x3_patch_chunk_stage"] and (l_cout in (32, 64) or l_cin == 32):
                    return fc.patch_id(pbn, 0, True, 32)
                return fc.patch_id(pbn, 3, True, 32)
            if l_cout in (32, 64):
                return fc.patch_id(l_cout, 3, True, 64)
            if l_cout % 256 == 0 and tiles * (l_cout // 256) >= opt["conv3x3_patch_min_workgroups"]:
                return fc.patch_id(256, 2, False, 64)
            return {1: fc.patch_id(128, 3, True, 64), 2: fc.patch_id(128, 4, True, 64), 0: fc.patch_id(128, 3, False, 64)}[opt["conv3x3_patch_unroll"]]
    if not k64:
        return fc.igemm_id(bn)
    stages = taps * (l_cin // 64)
    chunks = -(-l_cout // bn)
    pair = 1 < chunks <= 8
    if bn == 128 and stages <= 1:
        return fc.glds_id(128, 2, 4, pair=pair)
    if bn == 128 and stages <= 8:
        return fc.glds_id(128, 1, 4, pair=pair)
    assert not (l_cout % 128 == 0 and -(-n * ho * wo // 256) * (l_cout // 128) >= 512)
    return fc.glds_id(bn, 2 if bn == 128 else 3, pair=pair)
