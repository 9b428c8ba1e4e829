"""The dead-code revival of the EMA codebook (include/vqseg.h, EMA EXTENSION) restated on the CPU: the candidate hash in Python
integers, the candidate rows in NumPy and the update-with-expiry in float64 on top of the UNCHANGED oracle.torch_ref.vq_ema_update.
tests/test_vq_revive_cpu.py checks the restatement's own facts, tests/test_vq_revive_gpu.py holds the kernels and the module to it.

Bars.  A candidate row is a copy and the revived state is a copy, one fp32 multiply and a constant: bit for bit.  Which codes expire
is a comparison of the updated moving count with the threshold: every fixture is first shown (in float64) to keep every updated count
a relative 1e-4 away from the threshold, about a thousand times the two fp32 roundings of fmaf(cs, d, (1 - d) * n), so the float64
restatement and the fp32 kernel cannot disagree on the mask and no code is left out of a comparison.  Everything that is not revived is
today's update: bit-equal to vqseg_vq_ema_update_f32 on the same inputs and within the bars tests/vq_tail_cases.ema_reference counts."""
import contextlib
import functools

import numpy as np

from tests import vq_tail_cases as T

M64 = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB

# (seed, t, k) -> h, and (owner, j) at world * N = 600 (N = 300)
KNOWN = [((0, 0, 0), 0xe220a8397b1dcdaf, (1, 235)),
         ((0, 0, 1), 0x6e789e6aa1b965f4, (1, 0)),
         ((42, 0, 0), 0xbdd732262feb6e95, (0, 13)),
         ((42, 3, 511), 0xfe341aa0956ca61f, (1, 91)),
         (((1 << 64) - 1, (1 << 31) - 1, 65535), 0x5db664a6364077f1, (1, 149))]


def revive_hash(seed, t, k):
    """splitmix64 at counter t * 2^32 + k + 1"""
    x = (seed + GOLDEN * (t * (1 << 32) + k + 1)) & M64
    x = ((x ^ (x >> 30)) * MIX1) & M64
    x = ((x ^ (x >> 27)) * MIX2) & M64
    return x ^ (x >> 31)


def pick(seed, t, k, n, world):
    """-> (owner rank, row of that rank) of code k's candidate; every rank holds n rows"""
    return divmod(revive_hash(seed, t, k) % (world * n), n)


def candidates(rows, seed, t, n_codes, rank, world):
    """what vqseg_vq_revive_candidates writes on `rank`: rows (N, C) float32 = this rank's rows (bf16 rows: their float32 values)
    -> cand (K, C) float32 (the picked row where this rank owns it, else +0.0), ok (K,) float32"""
    rows = np.asarray(rows, dtype=np.float32)
    n, c = rows.shape
    cand, ok = np.zeros((n_codes, c), dtype=np.float32), np.zeros(n_codes, dtype=np.float32)
    for k in range(n_codes):
        owner, j = pick(seed, t, k, n, world)
        if owner == rank:
            cand[k] = rows[j]
            ok[k] = 1.0 if np.isfinite(rows[j]).all() else 0.0
    return cand, ok


def picked_rows(n, seed, t, n_codes, rank, world):
    """the rows of `rank` that some code picks (where a test plants its NaN / Inf)"""
    return [j for owner, j in (pick(seed, t, k, n, world) for k in range(n_codes)) if owner == rank]


# ---------------------------------------------------------------------------------------------------------------------
# the update with the expiry
# ---------------------------------------------------------------------------------------------------------------------
MASK_MARGIN = 1e-4
TAUS = (0.5, 2.0)
UPDATE_CASES = [(4, 4, 0.8), (33, 252, 0.8), (257, 260, 0.0), (1000, 516, 0.8), (256, 256, 1.0)]      # (K, C, decay)
SCENARIOS = ("none", "fifth", "all")


def assert_mask_is_safe(updated_cs64, tau, label):
    gap = np.abs(np.asarray(updated_cs64, dtype=np.float64) - tau)
    assert (gap > MASK_MARGIN * tau).all(), f"{label}: an updated moving count lies within {MASK_MARGIN} (relative) of the threshold {tau}"


@functools.lru_cache(maxsize=None)
def update_inputs(k, c, scenario):
    """-> rows (N, C) f32, idx (N,), counts (K,) i64, sums (K, C) f32, cluster_size (K,), embed_avg (K, C), cand (K, C), ok (K,).
    Integer member counts n and integer moving counts cs, chosen so that the updated count d cs + (1 - d) n meets neither threshold
    (0.5, 2.0) for any decay of UPDATE_CASES (0, 0.8, 1):
      "live" codes: n in {3, 4}, cs in {3, 4, 5}: updated count >= 3;
      "dead" codes: n in {0, 1}, cs in {0, 1}: updated count in {0, 0.2, 0.8, 1} -- below 2.0 always, below 0.5 for about half of them.
    "none": every code live; "fifth": max(1, K // 5) codes dead (tests/vq_tail_cases.ema_inputs' share of empty codes; its own counts
    put a code AT the threshold 2.0 for decay 0, so they cannot serve here); "all": every code dead and never a member, moving counts
    0 and 0.25 (updated count <= 0.25 < 0.5).
    Rows are multiples of 1/64, so the float32 sums are exact.  ok = 0 marks candidates that must revive nothing (none in "all", where
    S = 0 at decay 0 would put 0 / 0 into both entry points' codebooks)."""
    rs = np.random.RandomState(7000 + k + c)
    dead = np.zeros(k, dtype=bool)
    if scenario == "fifth":
        dead[rs.permutation(k)[:max(1, k // 5)]] = True
    elif scenario == "all":
        dead[:] = True
    counts = np.where(dead, rs.randint(0, 2, size=k), rs.randint(3, 5, size=k)).astype(np.int64)
    cs = np.where(dead, rs.randint(0, 2, size=k), rs.randint(3, 6, size=k)).astype(np.float32)
    first, second = np.flatnonzero(dead)[:1], np.flatnonzero(dead)[1:2]
    counts[first], cs[first], counts[second], cs[second] = 0, 0.0, 0, 0.0       # two codes that expire under either threshold
    if scenario == "all":
        counts[:] = 0
        cs = (0.25 * rs.randint(0, 2, size=k)).astype(np.float32)
    idx = rs.permutation(np.repeat(np.arange(k), counts)).astype(np.int64)
    rows = (rs.randint(-64, 65, size=(idx.size, c)) / 64.0).astype(np.float32)
    sums64 = np.zeros((k, c))
    np.add.at(sums64, idx, rows.astype(np.float64))
    sums = sums64.astype(np.float32)
    assert (sums.astype(np.float64) == sums64).all()
    avg = T.uniform(7100 + k + c, (k, c), -2.0, 2.0)
    cand = T.uniform(7200 + k + c, (k, c), -3.0, 3.0)
    ok = np.ones(k, dtype=np.float32)
    if scenario != "all":
        ok[::5] = 0.0
        ok[first] = 1.0
        ok[second] = 0.0                                                # an expired code whose candidate is unusable (K >= 10)
    out = rows, idx, counts, sums, cs, avg, cand, ok
    for a in out:
        a.setflags(write=False)
    return out


@contextlib.contextmanager
def _ema_inputs_are(inputs):
    """T.ema_reference counts its bars for the arrays T.ema_inputs hands it; the bars of another fixture are the SAME function on that
    fixture -- the source is neither copied nor changed"""
    keep = T.ema_inputs
    T.ema_inputs = lambda k, c, eps: inputs
    try:
        yield
    finally:
        T.ema_inputs = keep


def revive_reference(k, c, decay, tau, scenario, eps=T.EMA_EPS):
    """-> (expected, bars): expected = dict of float64 arrays cluster_size / embed_avg / codebook after the update with the expiry plus
    the bool mask `revived`; bars = T.ema_reference's {name: (ref, bound)} for the same inputs (what every non-revived entry is held to).
    Revived entries of `expected` are the exact values: tau, float32(s) * float32(tau), s."""
    rows, idx, counts, sums, cs, avg, cand, ok = update_inputs(k, c, scenario)
    with _ema_inputs_are((rows, idx, counts, sums, cs, avg)), np.errstate(divide="ignore", invalid="ignore"):     # "all": S may be 0
        bars = T.ema_reference(k, c, decay, eps)
    r_cs = bars["cluster_size"][0]
    assert_mask_is_safe(r_cs, tau, f"K {k} C {c} decay {decay} tau {tau} {scenario}")
    return apply_expiry(r_cs, bars["embed_avg"][0], bars["codebook"][0], cand, ok, tau), bars


def apply_expiry(r_cs, r_avg, r_cb, cand, ok, tau):
    """the rule of include/vqseg.h on the float64 result of oracle.torch_ref.vq_ema_update"""
    r_cs, r_avg, r_cb = (np.array(a, dtype=np.float64) for a in (r_cs, r_avg, r_cb))
    cand = np.asarray(cand, dtype=np.float32)
    revived = (r_cs < tau) & (np.asarray(ok) > 0)
    r_cs[revived] = np.float32(tau)
    r_avg[revived] = cand[revived] * np.float32(tau)                    # one fp32 multiply
    r_cb[revived] = cand[revived]
    return {"cluster_size": r_cs, "embed_avg": r_avg, "codebook": r_cb, "revived": revived}


def module_step_reference(cs, avg, rows_by_rank, idx, decay, eps, tau, seed, t):
    """one training forward's update of the MODULE, restated: oracle.torch_ref.vq_ema_update in float64 on all ranks' rows (float32
    values) under the assignment idx, then the expiry with the candidates the hash picks.  -> the dict of apply_expiry"""
    import torch
    from oracle import torch_ref as R
    rows = np.concatenate([np.asarray(r, dtype=np.float32) for r in rows_by_rank])
    k = np.asarray(cs).shape[0]
    t64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    r_cs, r_avg, r_cb = (v.numpy() for v in R.vq_ema_update(t64(cs), t64(avg), t64(rows), torch.from_numpy(np.array(idx, dtype=np.int64)),
                                                            float(np.float32(decay)), float(np.float32(eps))))
    assert_mask_is_safe(r_cs, tau, f"module step t = {t}")
    world = len(rows_by_rank)
    cand, ok = None, None
    for rank, shard in enumerate(rows_by_rank):
        ca, o = candidates(shard, seed, t, k, rank, world)
        cand, ok = (ca, o) if cand is None else (cand + ca, ok + o)
    return apply_expiry(r_cs, r_avg, r_cb, cand, ok, tau)
