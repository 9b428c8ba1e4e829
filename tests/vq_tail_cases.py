"""Cases, CPU references and assertion functions for the kernels that run after the argmin in csrc/vq_tail.hip and csrc/vq_codebook.hip: gather + finalize,
the two backward kernels, the member-list code sums (km_hist / km_scan / km_lists / km_segsum / km_sums / km_counts64), km_finalize and
the two EMA kernels.  Everything here is NumPy on the CPU: tests/test_vq_tail_gpu.py feeds the functions what the kernels returned,
tests/test_vq_tail_cpu.py feeds them order-faithful emulations and emulations that carry one defect each.

Bars.  None is fitted to a kernel's output; u = 2^-24.
  * whatever is a gather, a copy, a count or a chain of plain fp32 additions in a documented order: bit for bit;
  * the commitment loss: relative (all terms are squares), counted from vq_gather_kernel / vq_finalize_kernel (`loss_bar`);
  * the backward kernels: u |ref| + 4 u |k| |x - e| per element (`backward_ref`), bf16 outputs as the correctly rounded bf16 of the
    float64 reference with either neighbour allowed only within that bar of a rounding midpoint;
  * the code sums also against float64, depth u sum |x| (`sums_depth`), independently of the emulation;
  * the EMA update per element, counted from ema_counts_kernel / ema_embed_kernel (`ema_reference`).
Measured errors against these bars: profiles/vq_tail_parity.md."""
import functools

import numpy as np

U = 2.0 ** -24
GUARD = 64                                        # elements behind every output buffer that must keep their fill

# launch geometry of csrc/vq_tail.hip and csrc/vq_codebook.hip (constants: csrc/vq_internal.h) (the tests name the paths these decide; test_vq_tail_cpu.py holds them to the source)
GATHER_BLOCKS_MAX, GATHER_ROWS_PER_BLOCK, GATHER_RG = 2048, 16, 4
UNPACK_BLOCKS_MAX, UNPACK_ROWS_PER_BLOCK = 512, 1024
BWD_BLOCKS_MAX, BWD_THREADS = 4096, 256
KM_RB, KM_SEG = 1024, 128

# the bars of tests/test_vq_gpu.py that the counted bars here must stay below
OLD_LOSS_RTOL = 1e-5
OLD_SUMS_TOL = 1e-5
OLD_EMA = {"cluster_size": (1e-6, 1e-6), "embed_avg": (1e-5, 1e-5), "codebook": (1e-5, 1e-6)}     # (rtol, atol)


def note(family, what, err, bar):
    """every check prints its figure and its bar before it asserts (pytest -s: the source of profiles/vq_tail_parity.md)"""
    print(f"[{family}] {what}: {err:.3e} against {bar:.3e}" + (f" ({err / bar:.3f} of it)" if bar > 0 else ""))


# ---------------------------------------------------------------------------------------------------------------------
# number formats
# ---------------------------------------------------------------------------------------------------------------------
def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bf16_bits(a32):
    """round-to-nearest-even bf16 of finite float32 values, as uint16"""
    u = f32_bits(a32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_exact(a32):
    """the float32 values of the nearest bf16 numbers"""
    return bf16_to_f32(bf16_bits(a32))


def bf16_rne_f64(v):
    """float64 -> the nearest bf16 VALUE (ties to even), as float64: one rounding, not float64 -> float32 -> bf16"""
    m, e = np.frexp(np.asarray(v, dtype=np.float64))                  # v = m 2^e, |m| in [0.5, 1): 8 significand bits = rint(256 m)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def uniform(seed, shape, lo=-1.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, size=shape).astype(np.float32)


def guard_intact(tail, integer=False):
    """the GUARD elements behind an output: NaN (floats) or -1 (integers), every one"""
    tail = np.asarray(tail)
    assert tail.size == GUARD
    return bool((tail == -1).all()) if integer else bool(np.isnan(tail.astype(np.float64)).all())


# =====================================================================================================================
# 1. gather + finalize
# =====================================================================================================================
# name: (N, C of the fp32 rows, C of the bf16 rows (C % 8 == 0), K, what the case runs)
GATHER_CASES = {
    "one_row": (1, 4, 8, 1, "fewer rows than one row group (RG = 4): three of the four row slots of wave 0 are masked; K = 1"),
    "three_rows": (3, 8, 8, 5, "fewer rows than one row group; a workgroup whose waves 1..3 have nothing to do"),
    "ragged_second_channel_pass": (17, 260, 264, 7, "a ragged last row group (row 16 alone); C / 4 = 65 (66) > 64: lanes 0 (0..1) take a "
                                                    "second channel pass of the `v += 64` loop"),
    "one_block_past_the_cap": (32768 + 53, 8, 8, 33, "GATHER_BLOCKS_MAX = 2048 workgroups of 16 rows: rows 32768.. are the grid-stride second "
                                                     "pass of vq_gather_kernel, 53 rows = 13 groups and a ragged one"),
    "three_passes": (65541, 12, 16, 9, "more than two passes of the gather grid-stride loop (rows 65536.. are the third)"),
    "past_the_unpack_cap": (524288 + 1029, 4, 8, 40, "vq_unpack_keys' histogram launch is capped at 512 workgroups of 1024 rows (four "
                                                     "iterations of 256 threads): rows 524288.. are a fifth, strided by the capped grid (17 "
                                                     "gather passes); codes 35..39 lie far from every "
                                                     "row, so dead_pct >= 12.5 is read from that histogram"),
}
GATHER_CW = (0.0, 0.25, 1.0)
N_DEAD_FAR = 5


def gather_shape(name, bf16):
    n, c32, c16, k, _ = GATHER_CASES[name]
    return n, (c16 if bf16 else c32), k


@functools.lru_cache(maxsize=2)
def gather_inputs(name, bf16):
    """x (N, C) float32 (bf16 rows: bf16-exact values), W (K, C) float32 that is NOT bf16-exact (so the bf16 eval output is a rounding)"""
    n, c, k = gather_shape(name, bf16)
    seed = 1000 + 10 * sorted(GATHER_CASES).index(name) + int(bf16)
    x = uniform(seed, (n, c))
    if bf16:
        x = bf16_exact(x)
    w = uniform(seed + 5, (k, c))
    if name == "past_the_unpack_cap":
        w[-N_DEAD_FAR:] += 100.0
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def gather_blocks(n):
    return max(1, min(GATHER_BLOCKS_MAX, (n + GATHER_ROWS_PER_BLOCK - 1) // GATHER_ROWS_PER_BLOCK))


def gather_passes(n):
    """passes of the grid-stride loop of vq_gather_kernel that workgroup 0, wave 0 makes"""
    return (((n + GATHER_RG - 1) // GATHER_RG) + gather_blocks(n) * 4 - 1) // (gather_blocks(n) * 4)


def unpack_passes(n):
    """iterations of vq_unpack_keys' grid-stride loop (256 threads a workgroup): 4 up to the cap of 512 workgroups, more past it"""
    blocks = max(1, min(UNPACK_BLOCKS_MAX, (n + UNPACK_ROWS_PER_BLOCK - 1) // UNPACK_ROWS_PER_BLOCK))
    return (n + blocks * 256 - 1) // (blocks * 256)


def nearest_codes(x, w):
    """a valid idx for the CPU tests (float64 argmin); the GPU tests take the kernel's own idx -- assign has its own suites"""
    x, w = x.astype(np.float64), w.astype(np.float64)
    out = np.empty(x.shape[0], dtype=np.int64)
    for s in range(0, x.shape[0], 65536):
        xs = x[s:s + 65536]
        d = (xs * xs).sum(1)[:, None] + (w * w).sum(1)[None, :] - 2.0 * xs @ w.T
        out[s:s + 65536] = d.argmin(1)
    return out


def gather_expected(x, w, idx, training):
    """-> (q float32 BEFORE any bf16 store rounding, dlt float32): eval q = W[idx]; train q = x + (e - x) in float32 -- two roundings,
    no multiplication, so the compiler has nothing to contract -- and dlt = q - x in float32, the value the kernel squares"""
    e = w[idx]
    if not training:
        return e, None
    q = (x + (e - x).astype(np.float32)).astype(np.float32)
    return q, (q - x).astype(np.float32)


def loss_term_depths(n, c):
    """For every element (row, channel): the number of fp32 roundings its square passes through inside its lane's fmaf chain of
    vq_gather_kernel -- chain = (workgroup, wave, lane); order: grid-stride pass, channel pass (v += 64), row of the group, element of the
    float4.  The first term of a chain of L sees all L fmaf roundings, the last sees one."""
    c4 = c // 4
    nws = gather_blocks(n) * 4                                        # waves of the grid = row groups per pass
    r = np.arange(n, dtype=np.int64)
    g, j = r // GATHER_RG, r % GATHER_RG
    ws, p = g % nws, g // nws
    rows_in_group = np.minimum(GATHER_RG, n - g * GATHER_RG)          # only the very last group is ragged, and it is the last of its chain
    ch = np.arange(c, dtype=np.int64)
    v, i = ch // 4, ch % 4
    lane, cp = v % 64, v // 64
    ncp = (c4 - lane + 63) // 64                                      # channel passes of that lane
    rows_of_chain = np.bincount(ws, minlength=nws)[ws]
    chain_len = rows_of_chain[:, None] * 4 * ncp[None, :]
    pos = p[:, None] * (GATHER_RG * 4) * ncp[None, :] + cp[None, :] * (rows_in_group[:, None] * 4) + j[:, None] * 4 + i[None, :]
    return (chain_len - pos).astype(np.int32)


LOSS_TAIL_ROUNDINGS = 6 + 3 + 2            # six shuffle adds, (w0 + w1) + (w2 + w3): three adds, (float)(sd / numel) and * cw


def loss_ref(dlt, cw):
    """commitment_weight * mean(dlt^2) in float64 on the float32 dlt the kernel squares; cw is the float32 value the kernel receives"""
    d = dlt.astype(np.float64)
    return float(np.float32(cw)) * float((d * d).sum()) / d.size


def loss_bar(dlt):
    """-> (relative bar, plain count).  Counted from the source, each rounding worth u:
      plain count = the longest per-lane fmaf chain (loss_term_depths().max()) + six shuffle adds + three wave adds + the two final float
      roundings.  vq_finalize_kernel adds the workgroups' partials in double (2^-53 each: not counted).
    The plain count charges EVERY term the whole chain.  A term only sees the fmaf roundings that come after it, so the bar used is
      u (sum_i depth_i t_i / sum_i t_i + 11),   t_i = dlt_i^2 >= 0,
    first order in u like the plain count and never above it.  For past_the_unpack_cap the plain count is 17 passes x 16 + 11 = 283, i.e.
    1.7e-5 -- above the 1e-5 of tests/test_vq_gpu.py -- while the weighted count of its inputs is about half of that; the tests assert
    bar < 1e-5 for every case, and plain count x u < 1e-5 for the other five."""
    n, c = dlt.shape
    depth = loss_term_depths(n, c)
    t = dlt.astype(np.float64) ** 2
    plain = int(depth.max()) + LOSS_TAIL_ROUNDINGS
    weighted = float((depth * t).sum() / t.sum()) + LOSS_TAIL_ROUNDINGS
    assert weighted <= plain
    return weighted * U, plain


def emulate_gather_loss(dlt, cw, only_first_pass=False):
    """vq_gather_kernel's partial sums and vq_finalize_kernel's scalar in their order, in float32: per-lane fmaf chains, the xor-shuffle
    tree, the wave combine, the partials summed in double.  (The fma is formed in float64 and rounded to float32: a double rounding is
    possible, so this emulation is held to the float64 bar and not offered for bit equality.)
    only_first_pass: the defect `break after the first pass of the grid-stride loop`."""
    n, c = dlt.shape
    c4 = c // 4
    nb = gather_blocks(n)
    nws = nb * 4
    ncp = (c4 + 63) // 64
    lanes = c4 if ncp == 1 else 64
    npass = gather_passes(n)
    d = np.zeros((npass * nws * GATHER_RG, ncp * lanes * 4), dtype=np.float32)
    d[:n, :c] = dlt
    d = d.reshape(npass, nws, GATHER_RG, ncp, lanes, 4).transpose(1, 4, 0, 3, 2, 5).reshape(nws, lanes, -1)   # (wave, lane, chain)
    if only_first_pass:
        d = d[:, :, :ncp * GATHER_RG * 4]
    sq = np.zeros((nws, lanes), dtype=np.float32)
    for t in range(d.shape[2]):
        dt = d[:, :, t].astype(np.float64)
        sq = (dt * dt + sq.astype(np.float64)).astype(np.float32)     # a padded slot: fmaf(0, 0, sq) = sq
    wave = np.zeros((nws, 64), dtype=np.float32)
    wave[:, :lanes] = sq
    lane_id = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        wave = (wave + wave[:, lane_id ^ m]).astype(np.float32)
    ws = wave[:, 0].reshape(nb, 4)
    partial = ((ws[:, 0] + ws[:, 1]).astype(np.float32) + (ws[:, 2] + ws[:, 3]).astype(np.float32)).astype(np.float32)
    s = float(partial.astype(np.float64).sum())
    return np.float32(np.float32(s / (float(n) * float(c))) * np.float32(cw))


def check_gather(x, w, k, idx, training, cw, bf16, quant_bits, loss, dead_pct, label):
    """every assertion of section 1 on one forward call.  quant_bits: (N, C) uint32 (fp32 rows) or uint16 (bf16 rows); loss, dead_pct:
    float32 scalars.  Returns the loss error as a share of its bar (None where the loss is off)."""
    n, c = x.shape
    idx = np.asarray(idx)
    assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < k, f"{label}: idx outside [0, K)"
    q, dlt = gather_expected(x, w, idx, training)
    want = bf16_bits(q) if bf16 else f32_bits(q)
    quant_bits = np.asarray(quant_bits).reshape(n, c)
    bad = quant_bits != want
    if bad.any():
        rows = np.flatnonzero(bad.any(1))
        raise AssertionError(f"{label}: quant differs in {int(bad.sum())} elements of {rows.size} rows (first row {rows[0]}, last {rows[-1]}; "
                             f"rows from {gather_blocks(n) * GATHER_ROWS_PER_BLOCK} on belong to a later grid-stride pass)")
    zeros = int((np.bincount(idx, minlength=k) == 0).sum())
    want_dead = np.float32(100) * (np.float32(zeros) / np.float32(k))
    assert f32_bits(dead_pct) == f32_bits(want_dead), f"{label}: dead_pct {dead_pct!r}, expected {want_dead!r} ({zeros} of {k} codes unused)"
    loss = np.float32(loss)
    if not training or cw == 0:
        assert f32_bits(loss) == 0, f"{label}: loss {loss!r} where it must be +0.0"
        return None
    ref = loss_ref(dlt, cw)
    bar, plain = loss_bar(dlt)
    err = abs(float(loss) - ref) / ref
    note("gather", f"{label} loss (chain {plain - LOSS_TAIL_ROUNDINGS}, plain count {plain}, weighted {bar / U:.1f})", err, bar)
    assert bar < OLD_LOSS_RTOL, f"{label}: counted bar {bar:.3e} is not below {OLD_LOSS_RTOL}"
    assert err <= bar, f"{label}: loss {float(loss)!r} against {ref!r}: relative error {err:.3e} above the counted {bar:.3e}"
    return err / bar


# =====================================================================================================================
# 2. backward
# =====================================================================================================================
BWD_CASES = {
    False: [(1, 4), (3, 8), (64, 16), (65, 24), (257, 40), (2049, 2048)],
    True: [(1, 8), (3, 8), (64, 16), (65, 24), (257, 40), (2049, 2048)],
}
BWD_WHAT = {
    (1, 4): "smallest size: one float4, one thread", (1, 8): "smallest bf16 size: two float4 of one row",
    (3, 8): "six float4", (64, 16): "exactly 256 float4: one full workgroup",
    (65, 24): "C / 4 = 6, not a power of two: the `i / c4` row split of vq_backward_idx_kernel decides which code row is read",
    (257, 40): "ragged: 2570 float4, the last workgroup partly idle",
    (2049, 2048): "N C / 4 = 1 049 088 float4 = 512 past the 4096 x 256 grid cap: the grid-stride second pass of both backward kernels",
}
BWD_K = (1, 37)
BWD_GLOSS = (None, 0.7, -1.3)
BWD_CW = (0.0, 0.25)
MIDPOINT_SHARE_CAP = 1e-3


def bwd_strided(n, c):
    return n * c // 4 > BWD_BLOCKS_MAX * BWD_THREADS


@functools.lru_cache(maxsize=2)
def backward_inputs(n, c, k, bf16):
    """g, x (N, C) float32 (bf16: bf16-exact), idx (N) with codes 0 and K - 1 present (N = 1: K - 1 alone), W exactly (K, C)"""
    seed = 2000 + n + 7 * c + 13 * k + int(bf16)
    g, x, w = uniform(seed, (n, c)), uniform(seed + 1, (n, c), -2.0, 2.0), uniform(seed + 2, (k, c), -2.0, 2.0)
    if bf16:
        g, x = bf16_exact(g), bf16_exact(x)
    idx = np.random.RandomState(seed + 3).randint(0, k, size=n).astype(np.int64)
    idx[0] = 0
    idx[-1] = k - 1
    for a in (g, x, w, idx):
        a.setflags(write=False)
    return g, x, idx, w


def backward_ref(g, x, e, gloss, cw):
    """ref = g + k (x - e) in float64, k = gloss cw 2 / (N C) from the float32 gloss and cw the kernel receives -> (ref, bar).
    bar = u |ref| + 4 u |k| |x - e|, counted from launch_backward / launch_backward_idx and the kernels: coef = (float)(cw * 2.0 / (N C))
    is one rounding (the double arithmetic under it: 2^-53), k = gloss[0] * coef one, xv - qv one -- three on the product k (x - e),
    carried as 4 to cover their second-order terms -- and the fmaf rounds once, on the result."""
    n, c = g.shape
    k = float(np.float32(gloss)) * float(np.float32(cw)) * 2.0 / (float(n) * float(c))
    d = x.astype(np.float64) - e.astype(np.float64)
    ref = g.astype(np.float64) + k * d
    return ref, U * np.abs(ref) + 4 * U * abs(k) * np.abs(d)


def check_backward_f32(gx, g, x, e, gloss, cw, label):
    gx = np.asarray(gx, dtype=np.float32).reshape(g.shape)
    if gloss is None or cw == 0:
        assert (f32_bits(gx) == f32_bits(g)).all(), f"{label}: gx must be gq bit for bit without a loss gradient"
        return None
    ref, bar = backward_ref(g, x, e, gloss, cw)
    err = np.abs(gx.astype(np.float64) - ref)
    ratio = np.where(np.isfinite(err), err, np.inf) / bar
    note("backward f32", label, float(ratio.max()), 1.0)
    bad = ~(err <= bar)
    assert not bad.any(), (f"{label}: {int(bad.sum())} of {bad.size} elements outside u |ref| + 4 u |k| |x - e|; worst {float(ratio.max()):.3g} "
                           f"of it at flat index {int(ratio.argmax())}")
    return float(ratio.max())


def bf16_candidates(ref, bar):
    """-> (nearest bf16 of ref, of ref - bar, of ref + bar) as float64 values; an element is ambiguous where the last two differ"""
    return bf16_rne_f64(ref), bf16_rne_f64(ref - bar), bf16_rne_f64(ref + bar)


def midpoint_share(ref, bar):
    _, lo, hi = bf16_candidates(ref, bar)
    return float((lo != hi).mean())


def check_backward_bf16(gx_bits, g, x, e, gloss, cw, label):
    """the bf16 kernel against the float64 reference, never against the fp32 kernel: the output is the correctly rounded bf16 of ref;
    where ref lies within the fp32 bar of a bf16 rounding midpoint either neighbour passes, and such elements are at most 0.1 %"""
    gx_bits = np.asarray(gx_bits, dtype=np.uint16).reshape(g.shape)
    if gloss is None or cw == 0:
        assert (gx_bits == bf16_bits(g)).all(), f"{label}: gx must be gq bit for bit without a loss gradient"
        return None
    ref, bar = backward_ref(g, x, e, gloss, cw)
    mid, lo, hi = bf16_candidates(ref, bar)
    got = bf16_to_f32(gx_bits).astype(np.float64)
    amb = lo != hi
    share = float(amb.mean())
    note("backward bf16", f"{label} elements within the bar of a midpoint", share, MIDPOINT_SHARE_CAP)
    assert share <= MIDPOINT_SHARE_CAP, f"{label}: {share:.2e} of the elements are ambiguous"
    good = np.where(amb, (got == lo) | (got == hi), got == mid)
    assert good.all(), (f"{label}: {int((~good).sum())} of {good.size} elements are not the correctly rounded bf16 of the float64 reference "
                        f"(first at flat index {int(np.flatnonzero(~good.reshape(-1))[0])})")
    return share


# =====================================================================================================================
# 3. code sums, k-means
# =====================================================================================================================
def build_idx(n, sizes, forced, seed):
    """idx (N) with exactly sizes[code] members per code.  forced: [(first row, [codes of consecutive rows])] placed first; the rest of
    every cluster goes to the remaining rows in a seeded shuffle."""
    idx = np.full(n, -1, dtype=np.int64)
    left = dict(sizes)
    for start, codes in forced:
        codes = np.asarray(codes, dtype=np.int64)
        assert (idx[start:start + codes.size] == -1).all() and start + codes.size <= n
        idx[start:start + codes.size] = codes
        for code, cnt in zip(*np.unique(codes, return_counts=True)):
            left[int(code)] -= int(cnt)
    assert all(v >= 0 for v in left.values()), left
    rest = np.concatenate([np.full(v, code, dtype=np.int64) for code, v in sorted(left.items())] + [np.zeros(0, dtype=np.int64)])
    free = np.flatnonzero(idx < 0)
    assert rest.size == free.size, (rest.size, free.size)
    idx[free] = rest[np.random.RandomState(seed).permutation(rest.size)]
    return idx


def _sums_case(n, k, c32, c16, sizes, forced, claims, doc):
    assert sum(sizes.values()) == n
    return dict(n=n, k=k, c={False: c32, True: c16}, sizes=sizes, forced=forced, claims=claims, doc=doc)


_BIG = 3338
SUMS_CASES = {
    "n1": _sums_case(1, 1, 4, 8, {0: 1}, [], {}, "N = 1, K = 1: one member, one segment, one row block with 1023 idle rows"),
    "n63": _sums_case(63, 3, 60, 56, {0: 5, 2: 58}, [], {},
                      "N = 63 (less than one 64-row chunk of km_lists), K = 3 with code 1 empty, cluster of 5; C below one 64-channel group"),
    "n64_distinct": _sums_case(64, 64, 64, 64, {q: 1 for q in range(64)}, [(0, [(q * 37) % 64 for q in range(64)])],
                               {"distinct": [0]},
                               "N = 64: one chunk of 64 DISTINCT codes (64 rounds of the ballot loop of km_lists_kernel), C = 64"),
    "n65_alternating": _sums_case(65, 3, 68, 72, {0: 32, 1: 1, 2: 32}, [(0, [0, 2] * 32), (64, [1])], {"alternating": [0]},
                                  "N = 65: a chunk alternating codes 0 and 2 (ranks by popcount of every second lane), one row in a second "
                                  "chunk; C = 68 (72): a second 64-channel group of 4 (8) channels"),
    "n1023_sizes": _sums_case(1023, 1024, 4, 8, {**{3: 127, 4: 128, 5: 129, 900: 4, 901: 5, 7: 256, 1023: 257}, **{100 + q: 1 for q in range(117)}},
                              [], {}, "N = 1023, K = 1024 (km_scan: per = 1): clusters of 127 / 128 / 129 (one segment short, exact, one "
                                      "past), 256 / 257 (two segments, a third of one member), 4, 5 and 117 of one; code K - 1 populated"),
    "n1024_per2": _sums_case(1024, 1025, 64, 64, {7: 512, 600: 256, 1: 255, 1024: 1}, [(128, [7] * 64)], {"one_code": [128]},
                             "N = 1024 (exactly one row block), K = 1025: km_scan_kernel with per = 2, code K - 1 = 1024 owned by thread 512; "
                             "cluster of 512 = four full segments = one per thread row of km_sums; a 64-row chunk of one code"),
    "n1025_per3": _sums_case(1025, 2049, 132, 136, {**{2048: 513, 1500: 257, 1026: 129, 3: 62}, **{1100 + 5 * q: 1 for q in range(64)}},
                             [(960, [1100 + 5 * ((q * 11) % 64) for q in range(64)]), (1024, [2048])], {"distinct": [960], "spread": (2048, [1024])},
                             "N = 1025 (row 1024 alone in a second row block), K = 2049 > N: km_scan_kernel with per = 3, most codes empty; "
                             "cluster of 513 = five segments (thread row 0 of km_sums takes two) at C = 132 (136): three 64-channel groups, "
                             "the last of 4 (8) channels"),
    "n5197_blocks": _sums_case(5 * 1024 + 77, 64, 68, 72, {9: _BIG, 20: 641, 63: 513, 0: 512, 31: 128, 32: 64, 40: 1},
                               [(1023, [9, 9]), (5 * 1024 + 76, [9]), (2048, [32] * 64), (3072 + 64, [0, 63] * 32)],
                               {"one_code": [2048], "alternating": [3072 + 64], "spread": (9, [1023, 1024, 5 * 1024 + 76])},
                               "N = 5 x 1024 + 77: six row blocks, the cursors of km_scan across them; cluster of 3338 (27 segments) spread over "
                               "all six blocks with members at rows 1023, 1024 and N - 1; 641 = six segments (thread rows 0 and 1 of km_sums "
                               "take two); 513, 512; a chunk of one code, a chunk alternating two; C = 68 (72): two channel groups"),
}
REQUIRED_SIZES = (0, 1, 4, 5, 127, 128, 129, 256, 257, 512, 513, 641)
REQUIRED_N = (1, 63, 64, 65, 1023, 1024, 1025, 5 * 1024 + 77)
REQUIRED_K = (1, 3, 64, 1024, 1025, 2049)
REQUIRED_C = {False: (4, 60, 64, 68, 132), True: (8, 56, 64, 72, 136)}


@functools.lru_cache(maxsize=None)
def sums_idx(name):
    cs = SUMS_CASES[name]
    idx = build_idx(cs["n"], cs["sizes"], cs["forced"], seed=3000 + sorted(SUMS_CASES).index(name))
    idx.setflags(write=False)
    return idx


def dense_rows(seed, n, c, bf16):
    """dense, mixed-sign rows without zeros (0.25 <= |x| < 2), so every channel sees a dropped or doubled member.  bf16 rows are
    bf16-exact, and every element is scaled by one of 2^0 .. 2^-16: sums of 8-bit significands at ONE scale are exact in fp32 whatever
    the order; spread over 19 binades they round, so the bit comparison holds the order of a bf16 sum too."""
    rs = np.random.RandomState(seed)
    x = (rs.uniform(0.25, 2.0, size=(n, c)) * rs.choice([-1.0, 1.0], size=(n, c))).astype(np.float32)
    if bf16:
        x = bf16_exact(x) * np.ldexp(1.0, -rs.randint(0, 17, size=(n, c))).astype(np.float32)
    return x


@functools.lru_cache(maxsize=None)
def sums_rows(name, bf16):
    cs = SUMS_CASES[name]
    x = dense_rows(3100 + 2 * sorted(SUMS_CASES).index(name) + int(bf16), cs["n"], cs["c"][bf16], bf16)
    x.setflags(write=False)
    return x


def _fold4(acc):
    """((s0 + s1) + s2) + s3 over axis -2 of float32 (..., 4, C)"""
    return ((acc[..., 0, :] + acc[..., 1, :]) + acc[..., 2, :]) + acc[..., 3, :]


def _strided4(parts):
    """parts float32 (M, C), M items in order: four accumulators take items w, w + 4, ... (s = 0; s += item) and fold as _fold4"""
    m, c = parts.shape
    steps = (m + 3) // 4
    pad = np.zeros((steps * 4, c), dtype=np.float32)
    pad[:m] = parts
    pad = pad.reshape(steps, 4, c)
    acc = np.zeros((4, c), dtype=np.float32)
    for t in range(steps):
        acc = acc + pad[t]                                            # float32 + float32; a padded slot adds +0.0
    return _fold4(acc)


def emulate_code_sums(x, idx, k, drop_last_of_segment=False, twice=None, fold_all_from_first=False):
    """The documented order of the member-list reduction, in float32, plain additions only (so its bits are the kernels' bits):
    members in row order (km_lists is stable); segments of KM_SEG = 128 members; inside a segment the four waves' accumulators take
    members b + w, b + w + 4, ... and fold as ((s0 + s1) + s2) + s3 (km_segsum_kernel); a cluster's segment partials go the same way
    over the four thread rows of km_sums_kernel.  -> (sums (K, C) float32, counts (K) int64).
    Defects, one at a time: drop_last_of_segment (`m < e - 1` in km_segsum), twice = a row that is summed twice,
    fold_all_from_first (every thread row of km_sums starts at the cluster's first segment)."""
    n, c = x.shape
    counts = np.bincount(idx, minlength=k).astype(np.int64)
    order = np.argsort(idx, kind="stable")
    off = np.concatenate([[0], np.cumsum(counts)])
    sums = np.zeros((k, c), dtype=np.float32)
    for code in np.flatnonzero(counts):
        mem = order[off[code]:off[code + 1]]
        if twice is not None and twice in mem:
            mem = np.sort(np.concatenate([mem, [twice]]))
        rows = x[mem]
        partial = []
        for s in range(0, rows.shape[0], KM_SEG):
            seg = rows[s:s + KM_SEG]
            partial.append(_strided4(seg[:-1] if drop_last_of_segment else seg))
        partial = np.stack(partial)
        if fold_all_from_first:
            acc = np.zeros((4, c), dtype=np.float32)
            for w in range(4):
                for g in range(0, partial.shape[0], 4):
                    acc[w] = acc[w] + partial[g]
            sums[code] = _fold4(acc)
        else:
            sums[code] = _strided4(partial)
    return sums, counts


def sums_depth(counts):
    """additions on the longest path of a cluster of n members: ceil(min(n, 128) / 4) + 4 inside a segment (the accumulator chain and
    the fold, the first `0 + x` counted), ceil(ceil(n / 128) / 4) + 4 across the segments"""
    n = np.asarray(counts, dtype=np.int64)
    return (np.minimum(n, KM_SEG) + 3) // 4 + 4 + ((n + KM_SEG - 1) // KM_SEG + 3) // 4 + 4


def sums_ref64(x, idx, k):
    """-> (sum of the member rows, sum of their absolute values), float64 (K, C)"""
    ref, ab = np.zeros((k, x.shape[1])), np.zeros((k, x.shape[1]))
    x64 = x.astype(np.float64)
    np.add.at(ref, idx, x64)
    np.add.at(ab, idx, np.abs(x64))
    return ref, ab


def check_depth_bound(sums, x, idx, k, label):
    """|sums - ref64| <= depth u sum |x| per element, independent of the emulation; -> worst share of the bound"""
    counts = np.bincount(idx, minlength=k)
    ref, ab = sums_ref64(x, idx, k)
    bound = sums_depth(counts)[:, None] * U * ab
    err = np.abs(np.asarray(sums, dtype=np.float64).reshape(ref.shape) - ref)
    live = counts > 0
    ratio = np.where(np.isfinite(err[live]), err[live], np.inf) / bound[live]
    worst = float(ratio.max())
    note("code sums", f"{label} against float64, worst share of depth u sum|x| (depth up to {int(sums_depth(counts).max())})", worst, 1.0)
    assert int(sums_depth(counts).max()) * U < OLD_SUMS_TOL          # of sum |x|: below the 1e-5 of test_code_sums_match_one_hot_products
    assert worst <= 1.0, f"{label}: sums off by {worst:.3g} of the depth bound"
    return worst


def check_code_sums(sums, counts, x, idx, k, label):
    """every assertion of section 3 on one vqseg_vq_code_sums call: counts, exact zeros, the emulation's bits, the float64 bound"""
    n, c = x.shape
    sums = np.asarray(sums, dtype=np.float32).reshape(k, c)
    counts = np.asarray(counts, dtype=np.int64).reshape(k)
    want_counts = np.bincount(idx, minlength=k)
    assert (counts == want_counts).all(), f"{label}: counts differ from bincount(idx) at codes {np.flatnonzero(counts != want_counts)[:8]}"
    assert (f32_bits(sums[want_counts == 0]) == 0).all(), f"{label}: the sums row of an empty code is not +0.0"
    emu, _ = emulate_code_sums(x, idx, k)
    bad = f32_bits(sums) != f32_bits(emu)
    failed = []                                                       # both checks run, so a failure says which of the two caught it
    if bad.any():
        failed.append(f"sums differ from the order-faithful float32 emulation in {int(bad.sum())} elements of codes "
                      f"{np.flatnonzero(bad.any(1))[:8]} (sizes {want_counts[np.flatnonzero(bad.any(1))[:8]]})")
    worst = None
    try:
        worst = check_depth_bound(sums, x, idx, k, label)
    except AssertionError as e:
        failed.append(str(e))
    assert not failed, f"{label}: " + "; AND ".join(failed)
    return worst


def check_finalize(means, prev, sums, counts, label):
    """km_finalize_kernel: the correctly rounded fp32 quotient sums / float32(n) for populated codes (hipcc's default fp32 division is
    correctly rounded, the Makefile passes no fast-math flag); an empty code keeps its previous bits"""
    k, c = prev.shape
    means = np.asarray(means, dtype=np.float32).reshape(k, c)
    counts = np.asarray(counts).reshape(k)
    live = counts > 0
    want = prev.copy()
    want[live] = (sums[live] / counts[live].astype(np.float32)[:, None]).astype(np.float32)
    assert (f32_bits(means[~live]) == f32_bits(prev[~live])).all(), f"{label}: the mean of an empty code changed"
    bad = f32_bits(means) != f32_bits(want)
    assert not bad.any(), f"{label}: {int(bad.sum())} means are not the correctly rounded quotient (codes {np.flatnonzero(bad.any(1))[:8]})"


# =====================================================================================================================
# 4. EMA
# =====================================================================================================================
EMA_SHAPES = [(1, 4), (33, 252), (256, 256), (257, 260), (1000, 516)]          # (K, C)
EMA_DECAYS = (0.0, 0.8, 1.0)
EMA_EPS = 1e-5
EMA_CASES = [(k, c, d, EMA_EPS) for k, c in EMA_SHAPES for d in EMA_DECAYS] + [(33, 252, 0.8, 0.0)]


def ema_total_depth(k):
    """ema_counts_kernel: every thread's `s += v` chain (ceil(K / 256) additions) and the 8 levels of the LDS tree"""
    return (k + 255) // 256 + 8


@functools.lru_cache(maxsize=None)
def ema_inputs(k, c, eps):
    """-> rows (N, C) float32, idx (N), counts (K) int64, sums (K, C) float32, cluster_size (K), embed_avg (K, C).
    rows are multiples of 1/64 in [-1, 1] with at most four members per code, so their float64 sums ARE float32 numbers and the float32
    `sums` the kernel reads is exactly what oracle.torch_ref.vq_ema_update forms from rows and idx.  With eps > 0 a fifth of the codes
    (K > 1) are empty; some of those carry a moving count of 0 or 0.01 (codebook entries of magnitude 1e5 and 1e2).  With eps = 0 every
    code is populated."""
    rs = np.random.RandomState(4000 + k + c + (0 if eps else 1))
    populated = np.ones(k, dtype=bool)
    if eps > 0 and k > 1:
        populated[rs.permutation(k)[:max(1, k // 5)]] = False
    codes = np.flatnonzero(populated)
    idx = np.concatenate([codes, rs.choice(codes, size=k // 2 + 1)]).astype(np.int64)
    cnt = np.bincount(idx, minlength=k)
    while cnt.max() > 4:                                               # at most four members: the sums stay small and exact
        idx = np.delete(idx, np.flatnonzero(idx == cnt.argmax())[-1])
        cnt = np.bincount(idx, minlength=k)
    idx = idx[rs.permutation(idx.size)]
    rows = (rs.randint(-64, 65, size=(idx.size, c)) / 64.0).astype(np.float32)
    sums64 = np.zeros((k, c))
    np.add.at(sums64, idx, rows.astype(np.float64))
    sums = sums64.astype(np.float32)
    assert (sums.astype(np.float64) == sums64).all()
    cluster_size = rs.uniform(1.0, 3.0, size=k).astype(np.float32)
    empty = np.flatnonzero(~populated)
    cluster_size[empty[0::3]] = 0.0
    cluster_size[empty[1::3]] = 0.01
    embed_avg = uniform(4100 + k + c, (k, c), -2.0, 2.0)
    out = rows, idx, cnt.astype(np.int64), sums, cluster_size, embed_avg
    for a in out:
        a.setflags(write=False)
    return out


def ema_reference(k, c, decay, eps):
    """oracle.torch_ref.vq_ema_update in float64 on the float32 decay / eps the kernel receives, and the bars counted from the source.
    -> dict name: (ref, bound), float64.
      cluster_size = fmaf(cs, d, (1 - d) * (float)n): three roundings -- 1 - d, the product, the fma -- on |cs d| + |(1 - d) n|;
      embed_avg the same on |avg d| + |(1 - d) sums|;
      codebook = avg / smoothed, smoothed = (cs' + eps) / (S + (float)K * eps) * S with S the tree sum of cs' (relative error
      D + 3, D = ema_total_depth: all terms are non-negative): numerator 3 + 1, denominator (D + 3) + 1 + 1, the division 1, `* S`
      (D + 3) + 1, the last division 1: 2 D + 15 relative, carried as 2 D + 16 for the second-order terms, plus avg's own three
      roundings divided by smoothed."""
    import torch
    from oracle import torch_ref as R
    rows, idx, _, sums, cs, avg = ema_inputs(k, c, eps)
    d, e = float(np.float32(decay)), float(np.float32(eps))
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    r_cs, r_avg, r_cb = (v.numpy() for v in R.vq_ema_update(t(cs), t(avg), t(rows), torch.from_numpy(np.array(idx)), d, e))
    cnt = np.bincount(idx, minlength=k).astype(np.float64)
    s_cs = np.abs(cs.astype(np.float64) * d) + np.abs((1 - d) * cnt)
    s_avg = np.abs(avg.astype(np.float64) * d) + np.abs((1 - d) * sums.astype(np.float64))
    total = r_cs.sum()
    smoothed = (r_cs + e) / (total + k * e) * total
    depth = ema_total_depth(k)
    return {"cluster_size": (r_cs, 3 * U * s_cs), "embed_avg": (r_avg, 3 * U * s_avg),
            "codebook": (r_cb, (2 * depth + 16) * U * np.abs(r_cb) + 3 * U * s_avg / smoothed[:, None])}


def check_ema(k, c, decay, eps, cluster_size, embed_avg, codebook, total, label):
    """every assertion of section 4 on one vqseg_vq_ema_update_f32 call -> {name: worst share of its bar}"""
    _, _, counts, sums, cs0, avg0 = ema_inputs(k, c, eps)
    got = {"cluster_size": np.asarray(cluster_size, dtype=np.float32).reshape(k),
           "embed_avg": np.asarray(embed_avg, dtype=np.float32).reshape(k, c),
           "codebook": np.asarray(codebook, dtype=np.float32).reshape(k, c)}
    if decay == 1.0:                                                   # the exact facts first
        assert (f32_bits(got["cluster_size"]) == f32_bits(cs0)).all(), f"{label}: decay = 1 must keep cluster_size bit for bit"
        assert (f32_bits(got["embed_avg"]) == f32_bits(avg0)).all(), f"{label}: decay = 1 must keep embed_avg bit for bit"
    if decay == 0.0:
        assert (f32_bits(got["cluster_size"]) == f32_bits(counts.astype(np.float32))).all(), f"{label}: decay = 0: cluster_size != float(counts)"
        assert (f32_bits(got["embed_avg"]) == f32_bits(sums)).all(), f"{label}: decay = 0: embed_avg != sums bit for bit"
    worst = {}
    for name, (ref, bound) in ema_reference(k, c, decay, eps).items():
        rtol, atol = OLD_EMA[name]
        assert (bound <= atol + rtol * np.abs(ref)).all(), f"{label}: the counted bar of {name} is not below the old rtol {rtol} / atol {atol}"
        err = np.abs(got[name].astype(np.float64) - ref)
        ratio = np.where(bound > 0, np.where(np.isfinite(err), err, np.inf) / np.maximum(bound, 1e-300), np.where(err == 0, 0.0, np.inf))
        worst[name] = float(ratio.max())
        note("ema", f"{label} {name}", worst[name], 1.0)
        assert worst[name] <= 1.0, f"{label}: {name} off by {worst[name]:.3g} of its counted bar (flat index {int(ratio.argmax())})"
    # total: the kernel's own fp32 moving counts, summed in float64, against the tree's depth (all terms non-negative: relative)
    s = float(got["cluster_size"].astype(np.float64).sum())
    depth = ema_total_depth(k)
    err = abs(float(np.float32(total)) - s)
    note("ema", f"{label} total (depth {depth})", err, depth * U * s)
    assert depth * U < OLD_EMA["cluster_size"][0]
    assert err <= depth * U * s, f"{label}: total {float(total)!r} against {s!r}"
    worst["total"] = err / (depth * U * s) if s > 0 else 0.0
    return worst
