"""tests/vq_tail_cases.py without a GPU and without the library: its order-faithful emulations meet the float64 bounds on every case's
inputs, its assertion functions pass a float32 emulation of each kernel and reject that emulation carrying one defect at a time, the
midpoint cap of the bf16 backward check holds for the chosen inputs by the reference alone, and the constructed idx of every code-sum
case contains the cluster sizes and placements its description claims."""
import os
import re

import numpy as np
import pytest

from tests import vq_tail_cases as T

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vq_seg_amd", "csrc")
SRC = [os.path.join(CSRC, name) for name in ("vq_internal.h", "vq_tail.hip")]        # the geometry constants; the launchers of the tail


def fma32(a, b, c):
    """float32 fma through float64 (the product is exact there; the sum's double rounding is 2^-53 of it)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# the geometry the cases are built around is the source's
# ---------------------------------------------------------------------------------------------------------------------
def test_launch_geometry_is_the_sources():
    src = "".join(open(path).read() for path in SRC)
    const = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))
    assert (const("GATHER_BLOCKS_MAX"), const("GATHER_ROWS_PER_BLOCK"), const("KM_RB"), const("KM_SEG")) == \
        (T.GATHER_BLOCKS_MAX, T.GATHER_ROWS_PER_BLOCK, T.KM_RB, T.KM_SEG)
    for launch in ("hipError_t launch_backward(", "hipError_t launch_backward_idx("):                            # both backward launches
        body = src[src.index(launch):]
        body = body[:body.index("\n}\n")]
        assert f"if (blocks > {T.BWD_BLOCKS_MAX}) blocks = {T.BWD_BLOCKS_MAX};" in body and f"dim3({T.BWD_THREADS})" in body
    assert f"if (blocks > {T.UNPACK_BLOCKS_MAX}) blocks = {T.UNPACK_BLOCKS_MAX};" in src                        # vq_unpack_keys
    assert f"long blocks = (N[i] + {T.UNPACK_ROWS_PER_BLOCK - 1}) / {T.UNPACK_ROWS_PER_BLOCK};" in src


def test_cases_reach_the_paths_they_name():
    passes = {name: (T.gather_passes(v[0]), T.unpack_passes(v[0])) for name, v in T.GATHER_CASES.items()}
    assert passes == {"one_row": (1, 1), "three_rows": (1, 1), "ragged_second_channel_pass": (1, 1), "one_block_past_the_cap": (2, 4),
                      "three_passes": (3, 4), "past_the_unpack_cap": (17, 5)}       # unpack: 4 = 1024 rows a workgroup of 256, uncapped
    for name, (n, c32, c16, _, _) in T.GATHER_CASES.items():
        assert c32 % 4 == 0 and c16 % 8 == 0
    assert T.GATHER_CASES["ragged_second_channel_pass"][1] // 4 > 64 and 17 % T.GATHER_RG
    assert (32768 + 53) % T.GATHER_RG                                                  # the second pass itself ends ragged
    for bf16 in (False, True):
        assert [T.bwd_strided(n, c) for n, c in T.BWD_CASES[bf16]] == [False] * 5 + [True]
    assert 2049 * 2048 // 4 - T.BWD_BLOCKS_MAX * T.BWD_THREADS == 512
    assert (64 * 16 // 4, 24 // 4) == (256, 6)
    for k in T.BWD_K:                                                                  # codes 0 and K - 1 are read
        for n, c in T.BWD_CASES[True][1:]:
            idx = T.backward_inputs(n, c, k, True)[2]
            assert idx.min() == 0 and idx.max() == k - 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. gather: the loss chain emulation meets the bar; a skipped second pass is rejected
# ---------------------------------------------------------------------------------------------------------------------
def gather_emulated(name, bf16, training):
    x, w = T.gather_inputs(name, bf16)
    idx = T.nearest_codes(x, w)
    q, dlt = T.gather_expected(x, w, idx, training)
    bits = T.bf16_bits(q) if bf16 else T.f32_bits(q)
    zeros = int((np.bincount(idx, minlength=w.shape[0]) == 0).sum())
    return x, w, idx, bits, dlt, F(100) * (F(zeros) / F(w.shape[0]))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(T.GATHER_CASES))
def test_loss_chain_emulation_meets_the_counted_bar(name, bf16):
    x, w, idx, bits, dlt, dead = gather_emulated(name, bf16, 1)
    k = w.shape[0]
    if name == "past_the_unpack_cap":
        assert (np.bincount(idx, minlength=k)[-T.N_DEAD_FAR:] == 0).all() and dead >= 12.5
    for cw in (0.25, 1.0):
        share = T.check_gather(x, w, k, idx, 1, cw, bf16, bits, T.emulate_gather_loss(dlt, cw), dead, f"{name} emulated")
        assert share is not None and share <= 1.0
    bar, plain = T.loss_bar(dlt)
    assert bar < T.OLD_LOSS_RTOL and bar <= plain * T.U
    chain = {"one_row": 4, "three_rows": 12, "ragged_second_channel_pass": 2 * 16, "one_block_past_the_cap": 2 * 16, "three_passes": 3 * 16,
             "past_the_unpack_cap": 17 * 16}[name]                                       # rows x 4 elements x channel passes x passes
    assert plain == chain + T.LOSS_TAIL_ROUNDINGS
    assert (plain * T.U < T.OLD_LOSS_RTOL) == (name != "past_the_unpack_cap")
    assert T.check_gather(x, w, k, idx, 1, 0.0, bf16, bits, F(0), dead, name) is None
    e_bits = T.bf16_bits(w[idx]) if bf16 else T.f32_bits(w[idx])
    assert T.check_gather(x, w, k, idx, 0, 1.0, bf16, e_bits, F(0), dead, name) is None
    with pytest.raises(AssertionError, match="loss"):
        T.check_gather(x, w, k, idx, 0, 1.0, bf16, e_bits, F(1e-30), dead, name)             # the loss must be +0.0 exactly in eval
    with pytest.raises(AssertionError, match="dead_pct"):
        T.check_gather(x, w, k, idx, 0, 1.0, bf16, e_bits, F(0), np.nextafter(dead, F(200)), name)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["one_block_past_the_cap", "three_passes"])
def test_a_skipped_second_gather_pass_is_rejected(name, bf16):
    """the strided second pass skipped: the rows from 32 768 on stay NaN (the pre-fill) and their squares are missing from the loss"""
    x, w, idx, bits, dlt, dead = gather_emulated(name, bf16, 1)
    k = w.shape[0]
    first = T.gather_blocks(x.shape[0]) * T.GATHER_ROWS_PER_BLOCK
    assert first == 32768 < x.shape[0]
    good_loss = T.emulate_gather_loss(dlt, 0.25)
    unwritten = bits.copy()
    unwritten[first:] = 0x7FC0 if bf16 else 0x7FC00000
    with pytest.raises(AssertionError, match="quant differs"):
        T.check_gather(x, w, k, idx, 1, 0.25, bf16, unwritten, good_loss, dead, name)
    with pytest.raises(AssertionError, match="loss"):
        T.check_gather(x, w, k, idx, 1, 0.25, bf16, bits, T.emulate_gather_loss(dlt, 0.25, only_first_pass=True), dead, name)
    one_row = bits.copy()
    one_row[-1, -1] ^= 1                                                                 # one ulp in the very last element
    with pytest.raises(AssertionError, match="quant differs"):
        T.check_gather(x, w, k, idx, 1, 0.25, bf16, one_row, good_loss, dead, name)


def test_bf16_rounding_helpers():
    import torch
    a = T.uniform(7, (4096,), -3.0, 3.0)
    a[:4] = [1.00390625, 1.01171875, -1.00390625, 0.0]                                   # ties: to even
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (T.bf16_bits(a) == want).all()
    assert (T.bf16_rne_f64(a.astype(np.float64)) == T.bf16_exact(a).astype(np.float64)).all()
    assert T.bf16_rne_f64(1.00390625 + 2.0 ** -40) == 1.0078125 and T.bf16_rne_f64(1.00390625) == 1.0   # one rounding, not two


# ---------------------------------------------------------------------------------------------------------------------
# 2. backward: a float32 emulation passes, coef without its factor 2 does not; the midpoint cap by the reference alone
# ---------------------------------------------------------------------------------------------------------------------
def emulate_backward(g, x, e, gloss, cw, factor=2.0):
    n, c = g.shape
    coef = F(float(F(cw)) * factor / (float(n) * float(c)))
    k = F(0) if gloss is None else F(F(gloss) * coef)
    return fma32(k, (x - e).astype(F), g)


@pytest.mark.parametrize("n,c", T.BWD_CASES[False])
def test_backward_f32_check_passes_the_emulation_and_rejects_half_the_coefficient(n, c):
    g, x, idx, w = T.backward_inputs(n, c, 37, False)
    e = w[idx]
    for gloss in T.BWD_GLOSS:
        for cw in T.BWD_CW:
            T.check_backward_f32(emulate_backward(g, x, e, gloss, cw), g, x, e, gloss, cw, f"({n}, {c}) emulated")
            if gloss is not None and cw:
                with pytest.raises(AssertionError, match="outside"):
                    T.check_backward_f32(emulate_backward(g, x, e, gloss, cw, factor=1.0), g, x, e, gloss, cw, "coef without the factor 2")
    with pytest.raises(AssertionError, match="bit for bit"):
        T.check_backward_f32(np.nextafter(g, F(9)), g, x, e, None, 0.25, "one ulp off")
    unwritten = emulate_backward(g, x, e, 0.7, 0.25)
    unwritten[-1, -1] = np.nan
    with pytest.raises(AssertionError, match="outside"):
        T.check_backward_f32(unwritten, g, x, e, 0.7, 0.25, "last element left NaN")


@pytest.mark.parametrize("k", T.BWD_K)
@pytest.mark.parametrize("n,c", T.BWD_CASES[True])
def test_backward_bf16_check_and_midpoint_cap(n, c, k):
    """the 0.1 % cap on elements within the fp32 bar of a bf16 rounding midpoint, from the float64 reference alone, for every input the
    GPU test uses; the check passes the rounded float32 emulation and rejects coef without its factor 2 at every shape -- at
    (2049, 2048), where k is 1e-7, through the few hundred elements whose |g| is small enough for k (x - e) to move their bf16"""
    g, x, idx, w = T.backward_inputs(n, c, k, True)
    e = w[idx]
    for gloss in T.BWD_GLOSS[1:]:
        ref, bar = T.backward_ref(g, x, e, gloss, 0.25)
        assert T.midpoint_share(ref, bar) <= T.MIDPOINT_SHARE_CAP
        T.check_backward_bf16(T.bf16_bits(emulate_backward(g, x, e, gloss, 0.25)), g, x, e, gloss, 0.25, f"({n}, {c}) K={k} emulated")
        with pytest.raises(AssertionError, match="correctly rounded"):
            T.check_backward_bf16(T.bf16_bits(emulate_backward(g, x, e, gloss, 0.25, factor=1.0)), g, x, e, gloss, 0.25, "coef / 2")
    T.check_backward_bf16(T.bf16_bits(g), g, x, e, None, 0.25, "no loss gradient")
    T.check_backward_bf16(T.bf16_bits(g), g, x, e, 0.7, 0.0, "cw = 0")
    if n > 1 and k > 1:                                                                  # the neighbouring code row instead of the right one
        wrong = w[np.where(idx > 0, idx - 1, 1)]
        with pytest.raises(AssertionError, match="correctly rounded"):
            T.check_backward_bf16(T.bf16_bits(emulate_backward(g, x, wrong, -1.3, 0.25)), g, x, e, -1.3, 0.25, "wrong code row")


# ---------------------------------------------------------------------------------------------------------------------
# 3. code sums
# ---------------------------------------------------------------------------------------------------------------------
def test_constructed_idx_holds_the_claimed_sizes_and_placements():
    sizes, ns, ks = set(), set(), set()
    cs_of = {False: set(), True: set()}
    placements = set()
    for name, cs in T.SUMS_CASES.items():
        idx = T.sums_idx(name)
        n, k = cs["n"], cs["k"]
        assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < k
        counts = np.bincount(idx, minlength=k)
        assert {q: int(v) for q, v in enumerate(counts) if v} == cs["sizes"]
        sizes |= set(int(v) for v in counts)
        ns.add(n), ks.add(k), cs_of[False].add(cs["c"][False]), cs_of[True].add(cs["c"][True])
        assert cs["c"][False] % 4 == 0 and cs["c"][True] % 8 == 0
        for kind, where in cs["claims"].items():
            placements.add(kind)
            if kind == "spread":
                code, rows = where
                assert (idx[rows] == code).all()
                blocks = np.unique(np.flatnonzero(idx == code) // T.KM_RB)
                if name == "n5197_blocks":
                    assert blocks.size >= 3 and set(rows) == {1023, 1024, n - 1}
                continue
            for start in where:
                assert start % 64 == 0                                                   # a whole chunk of km_lists_kernel
                chunk = idx[start:start + 64]
                if kind == "one_code":
                    assert np.unique(chunk).size == 1
                elif kind == "alternating":
                    assert chunk[0] != chunk[1] and (chunk[0::2] == chunk[0]).all() and (chunk[1::2] == chunk[1]).all()
                elif kind == "distinct":
                    assert np.unique(chunk).size == 64
    assert set(T.REQUIRED_SIZES) <= sizes and max(sizes) > 3 * 1024
    assert ns == set(T.REQUIRED_N) and ks == set(T.REQUIRED_K)
    assert cs_of[False] == set(T.REQUIRED_C[False]) and cs_of[True] == set(T.REQUIRED_C[True])
    assert placements == {"one_code", "alternating", "distinct", "spread"}
    big = T.SUMS_CASES["n5197_blocks"]
    assert T.sums_depth([641])[0] == 32 + 4 + 2 + 4 and -(-641 // T.KM_SEG) == 6 and -(-513 // T.KM_SEG) == 5 and big["c"][False] > 64
    assert [(k + 1023) // 1024 for k in (1024, 1025, 2049)] == [1, 2, 3]               # km_scan_kernel's `per`


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(T.SUMS_CASES))
def test_sums_emulation_meets_the_depth_bound_and_defects_are_rejected(name, bf16):
    cs = T.SUMS_CASES[name]
    x, idx, k = T.sums_rows(name, bf16), T.sums_idx(name), cs["k"]
    assert (x != 0).all() and (bf16 or (np.abs(x) >= 0.25).all()) and (not bf16 or (T.bf16_exact(x) == x).all())
    sums, counts = T.emulate_code_sums(x, idx, k)
    worst = T.check_code_sums(sums, counts, x, idx, k, f"{name} emulated")
    assert worst < 0.5
    broken = {"the last member of a segment dropped": T.emulate_code_sums(x, idx, k, drop_last_of_segment=True)[0],
              "a member counted twice": T.emulate_code_sums(x, idx, k, twice=int(idx.size - 1))[0],
              "segments folded from the wrong start": T.emulate_code_sums(x, idx, k, fold_all_from_first=True)[0]}   # (one segment: four times)
    for what, bad in broken.items():
        with pytest.raises(AssertionError, match="emulation.*AND.*depth bound"):
            T.check_code_sums(bad, counts, x, idx, k, what)
        with pytest.raises(AssertionError, match="depth bound"):
            T.check_depth_bound(bad, x, idx, k, what)
    wrong_counts = counts.copy()
    wrong_counts[idx[0]] += 1
    with pytest.raises(AssertionError, match="counts"):
        T.check_code_sums(sums, wrong_counts, x, idx, k, "a count off by one")
    if (counts == 0).any():
        dirty = sums.copy()
        dirty[np.flatnonzero(counts == 0)[-1], -1] = -0.0
        with pytest.raises(AssertionError, match="empty"):
            T.check_code_sums(dirty, counts, x, idx, k, "an empty code's row not +0.0")


def test_depth_bound_has_the_margins_the_design_quotes():
    """a 3338-member cluster: the emulation's error is a small share of depth u sum |x|, one dropped member is tens to hundreds of times over it"""
    cs = T.SUMS_CASES["n5197_blocks"]
    x, idx, k = T.sums_rows("n5197_blocks", False), T.sums_idx("n5197_blocks"), cs["k"]
    only = idx == 9
    xs, ids = x[only], np.zeros(int(only.sum()), dtype=np.int64)
    assert ids.size == 3338
    good = T.check_depth_bound(T.emulate_code_sums(xs, ids, 1)[0], xs, ids, 1, "3338 members")
    assert good < 0.25
    ref, ab = T.sums_ref64(xs, ids, 1)
    dropped = np.abs(xs[-1].astype(np.float64)) / (T.sums_depth([3338])[0] * T.U * ab[0])
    assert dropped.min() > 20 and np.median(dropped) > 100


def test_finalize_check():
    counts = np.array([0, 1, 3, 7, 641, 0], dtype=np.int64)
    sums, prev = T.uniform(1, (6, 8), -50, 50), T.uniform(2, (6, 8))
    means = prev.copy()
    means[counts > 0] = sums[counts > 0] / counts[counts > 0].astype(F)[:, None]
    T.check_finalize(means, prev, sums, counts, "emulated")
    bad = means.copy()
    bad[0, 0] = 0.0
    with pytest.raises(AssertionError, match="empty"):
        T.check_finalize(bad, prev, sums, counts, "an empty code overwritten")
    bad = means.copy()
    sums[3, 0] = 3.0                                                                     # 3 / 7 = 0x3edb6db7; 3 * float32(1 / 7) = 0x3edb6db8
    means[3, 0] = F(3.0) / F(7.0)
    bad = means.copy()
    bad[3] = sums[3] * (F(1.0) / F(7.0))                                                 # reciprocal-multiply: one ulp off the rounded quotient
    assert T.f32_bits(bad[3, 0]) == 0x3EDB6DB8 and T.f32_bits(means[3, 0]) == 0x3EDB6DB7
    T.check_finalize(means, prev, sums, counts, "emulated")
    with pytest.raises(AssertionError, match="quotient"):
        T.check_finalize(bad, prev, sums, counts, "x * (1 / n)")


# ---------------------------------------------------------------------------------------------------------------------
# 4. EMA
# ---------------------------------------------------------------------------------------------------------------------
def emulate_ema(k, c, decay, eps, counts_term_decay=False):
    """ema_counts_kernel + ema_embed_kernel in float32, in their order; counts_term_decay: the defect `(1 - decay)` -> `decay` on counts"""
    _, _, counts, sums, cs0, avg0 = T.ema_inputs(k, c, eps)
    d, e = F(decay), F(eps)
    om = F(F(1) - d)
    cs = fma32(cs0, d, (d if counts_term_decay else om) * counts.astype(F))
    per = np.zeros(((k + 255) // 256, 256), dtype=F)
    per.reshape(-1)[:k] = cs
    s = np.zeros(256, dtype=F)
    for row in per:
        s = s + row
    w = 128
    while w:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    n = s[0]
    smoothed = ((cs + e) / (n + F(k) * e) * n).astype(F)
    avg = fma32(avg0, d, om * sums)
    return cs, avg, (avg / smoothed[:, None]).astype(F), n


@pytest.mark.parametrize("k,c,decay,eps", T.EMA_CASES)
def test_ema_check_passes_the_emulation_and_rejects_a_wrong_counts_weight(k, c, decay, eps):
    rows, idx, counts, sums, cs0, avg0 = T.ema_inputs(k, c, eps)
    assert idx.min() >= 0 and idx.max() < k and (counts == np.bincount(idx, minlength=k)).all()
    if eps == 0:
        assert (counts > 0).all()
    elif k > 1:
        assert (counts == 0).any() and (cs0[counts == 0] == 0).any()
    label = f"K={k} C={c} decay={decay} eps={eps} emulated"
    worst = T.check_ema(k, c, decay, eps, *emulate_ema(k, c, decay, eps), label)
    assert max(worst.values()) <= 1.0
    if decay == 0.8:
        with pytest.raises(AssertionError):
            T.check_ema(k, c, decay, eps, *emulate_ema(k, c, decay, eps, counts_term_decay=True), "counts weighted by decay")
    cs, avg, cb, n = emulate_ema(k, c, decay, eps)
    with pytest.raises(AssertionError, match="total"):
        T.check_ema(k, c, decay, eps, cs, avg, cb, F(n * F(1.0001)), "total off by 1e-4")
