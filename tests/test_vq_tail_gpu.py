"""Direct parity of the kernels that run after the argmin in csrc/vq_tail.hip and csrc/vq_codebook.hip -- vq_gather_kernel<float | bf16> + vq_finalize_kernel,
vq_backward_kernel, vq_backward_idx_kernel, the member-list code sums (km_hist / km_scan / km_lists / km_segsum / km_sums / km_counts64),
km_finalize_kernel, ema_counts_kernel + ema_embed_kernel -- through the C ABI, against NumPy / torch computations on the CPU of the same
inputs (tests/vq_tail_cases.py: cases, references, bars and the assertion functions; tests/test_vq_tail_cpu.py runs those functions on
emulated and deliberately broken results).

Every output buffer starts as NaN (integers: -1) with 64 guard elements behind it that must keep that fill.  Every idx fed to a kernel
lies in [0, K) and every input is finite: out-of-range codes and non-finite rows are tests/test_vq_nonfinite_gpu.py's subject.
Measured figures: profiles/vq_tail_parity.md (`pytest -s tests/test_vq_tail_gpu.py` prints each before it asserts)."""
import numpy as np
import pytest
import torch

from tests import vq_tail_cases as T
from tests.test_nn_kernels_gpu import BF16, F32, dev, lib, nan_like, ok, ptr, stream

pytestmark = pytest.mark.gpu
G = T.GUARD


def up(a, dtype=None):
    """a CPU array (read-only ones included) -> a device tensor of its own; bf16: the values are bf16-exact, the cast is exact"""
    t = torch.tensor(np.asarray(a)).to(dev())
    return t if dtype is None else t.to(dtype)


def out(n, dtype):
    return nan_like((n + G,), dtype)


def down(t, n, what):
    """-> the first n elements as NumPy (bf16: its uint16 bits), after checking the guard behind them"""
    torch.cuda.synchronize()
    body, tail = t[:n], t[n:]
    assert T.guard_intact(tail.float().cpu().numpy() if tail.is_floating_point() else tail.cpu().numpy(), integer=not tail.is_floating_point()), \
        f"{what}: the guard elements behind the output were written"
    if t.dtype == BF16:
        return body.view(torch.int16).cpu().numpy().view(np.uint16)
    return body.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. gather + finalize
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(T.GATHER_CASES))
def test_gather_and_finalize(name, bf16):
    """vqseg_vq_forward_f32 / _bf16 at the shapes of T.GATHER_CASES (each entry says which path it runs: row groups of fewer than four
    rows, the second channel pass, the grid-stride passes of vq_gather_kernel past GATHER_BLOCKS_MAX x 16 = 32 768 rows -- the loop every
    benchmarked step runs at 131 072 rows -- and of vq_unpack_keys past 512 x 1024 rows), training 0 / 1, commitment weight 0 / 0.25 / 1.
    eval: quant bits = W[idx] (bf16: its RNE rounding); train: bits of the float32 x + (e - x); loss against float64 within the counted
    relative bar (T.loss_bar), +0.0 exactly when off; dead_pct bits.  A row the kernel never wrote stays NaN and fails the bit check."""
    x, w = T.gather_inputs(name, bf16)
    (n, c), k = x.shape, w.shape[0]
    L, dt = lib(), BF16 if bf16 else F32
    print(f"[gather] {name}: {T.GATHER_CASES[name][4]} -- {T.gather_passes(n)} gather passes, {T.unpack_passes(n)} unpack passes")
    xd, wd = up(x, dt), up(w)
    nbytes = L.vqseg_vq_workspace_bytes(n, c, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    fn = L.vqseg_vq_forward_bf16 if bf16 else L.vqseg_vq_forward_f32
    for training in (0, 1):
        for cw in T.GATHER_CW:
            quant, idx, loss, dead = out(n * c, dt), out(n, torch.int64), out(1, F32), out(1, F32)
            ok(fn(ptr(xd), ptr(wd), None, n, c, k, training, cw, ptr(quant), ptr(idx), ptr(loss), ptr(dead), None, ptr(ws), nbytes, stream()))
            label = f"{name} {'bf16' if bf16 else 'f32'} training={training} cw={cw}"
            q = down(quant, n * c, label)
            q_bits = q if bf16 else q.view(np.uint32)
            idx_h = down(idx, n, label)
            if name == "past_the_unpack_cap":
                assert (np.bincount(idx_h, minlength=k)[-T.N_DEAD_FAR:] == 0).all(), "the far codes must stay dead"
            T.check_gather(x, w, k, idx_h, training, cw, bf16, q_bits, down(loss, 1, label)[0], down(dead, 1, label)[0], label)


# ---------------------------------------------------------------------------------------------------------------------
# 2. backward
# ---------------------------------------------------------------------------------------------------------------------
def gloss_tensor(gloss):
    return None if gloss is None else torch.tensor([gloss], dtype=F32, device=dev())


@pytest.mark.parametrize("n,c", T.BWD_CASES[False])
def test_backward_f32(n, c):
    """vqseg_vq_backward_f32 (vq_backward_kernel) at T.BWD_CASES -- (2049, 2048) is 512 float4 past the 4096-workgroup cap, the grid-stride
    second pass -- with grad_loss NULL / +0.7 / -1.3 and commitment weight 0 / 0.25.  Without a loss gradient gx = gq bit for bit; otherwise
    against g + k (x - q) in float64 within u |ref| + 4 u |k| |x - q| (T.backward_ref counts the roundings from the source)."""
    g, x, idx, w = T.backward_inputs(n, c, 37, False)
    e = w[idx]
    print(f"[backward f32] ({n}, {c}): {T.BWD_WHAT[(n, c)]}")
    gd, xd, qd = up(g), up(x), up(e)
    for gloss in T.BWD_GLOSS:
        for cw in T.BWD_CW:
            gx = out(n * c, F32)
            gl = gloss_tensor(gloss)
            ok(lib().vqseg_vq_backward_f32(ptr(gd), ptr(gl), ptr(xd), ptr(qd), n, c, cw, ptr(gx), stream()))
            label = f"({n}, {c}) gloss={gloss} cw={cw}"
            T.check_backward_f32(down(gx, n * c, label), g, x, e, gloss, cw, label)


@pytest.mark.parametrize("k", T.BWD_K)
@pytest.mark.parametrize("n,c", T.BWD_CASES[True])
def test_backward_bf16(n, c, k):
    """vqseg_vq_backward_bf16 (vq_backward_idx_kernel) at T.BWD_CASES, K = 1 and 37 with codes 0 and K - 1 among idx and the codebook
    allocated at exactly K C floats, so the `i / c4` row split and the W + idx C address are held at both ends; (2049, 2048) runs the
    grid-stride second pass.  Judged against the float64 reference g + k (x - W[idx]) -- never against the fp32 kernel, so a mistake in
    coef or gloss shared by both kernels fails: the output is the correctly rounded bf16 of it, either neighbour only within the fp32 bar
    of a rounding midpoint, at most 0.1 % of the elements."""
    g, x, idx, w = T.backward_inputs(n, c, k, True)
    e = w[idx]
    print(f"[backward bf16] ({n}, {c}), K = {k}: {T.BWD_WHAT[(n, c)]}")
    gd, xd, idxd, wd = up(g, BF16), up(x, BF16), up(idx), up(w)
    assert wd.numel() == k * c
    for gloss in T.BWD_GLOSS:
        for cw in T.BWD_CW:
            gx = out(n * c, BF16)
            gl = gloss_tensor(gloss)
            ok(lib().vqseg_vq_backward_bf16(ptr(gd), ptr(gl), ptr(xd), ptr(idxd), ptr(wd), n, c, cw, ptr(gx), stream()))
            label = f"({n}, {c}) K={k} gloss={gloss} cw={cw}"
            T.check_backward_bf16(down(gx, n * c, label), g, x, e, gloss, cw, label)


# ---------------------------------------------------------------------------------------------------------------------
# 3. code sums, k-means
# ---------------------------------------------------------------------------------------------------------------------
def code_sums(xd, idxd, n, c, k, bf16, label):
    L = lib()
    nbytes = L.vqseg_kmeans_workspace_bytes(n, c, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    sums, counts = out(k * c, F32), out(k, torch.int64)
    ok(L.vqseg_vq_code_sums(int(bf16), ptr(xd), ptr(idxd), n, c, k, ptr(sums), ptr(counts), ptr(ws), nbytes, stream()))
    return down(sums, k * c, label).reshape(k, c), down(counts, k, label)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(T.SUMS_CASES))
def test_code_sums_constructed_clusters(name, bf16):
    """vqseg_vq_code_sums on CONSTRUCTED idx (T.SUMS_CASES; each entry says what it runs): cluster sizes 0, 1, 4, 5, 127, 128, 129, 256,
    257, 512, 513, 641 and 3338 -- one segment short / exact / past, km_sums_kernel's thread rows taking one and two segments, more than
    four segments over several 64-channel groups, fp32 and bf16 rows -- km_scan_kernel with per = 1, 2 and 3, and km_lists_kernel's
    ballot ranking on a chunk of one code, of two alternating codes and of 64 distinct codes and its cursors across six row blocks.
    counts = bincount; empty codes' sums +0.0; sums bit-equal to the order-faithful float32 emulation of the documented order; and,
    independently, within depth u sum |x| of float64.  km_finalize_kernel on the same sums: correctly rounded quotients, empty codes keep
    their means."""
    cs = T.SUMS_CASES[name]
    n, k, c = cs["n"], cs["k"], cs["c"][bf16]
    x, idx = T.sums_rows(name, bf16), T.sums_idx(name)
    label = f"{name} {'bf16' if bf16 else 'f32'}"
    print(f"[code sums] {label} (N {n}, C {c}, K {k}): {cs['doc']}")
    sums, counts = code_sums(up(x, BF16 if bf16 else F32), up(idx), n, c, k, bf16, label)
    T.check_code_sums(sums, counts, x, idx, k, label)
    prev = T.uniform(5000 + n, (k, c), -3.0, 3.0)
    means = out(k * c, F32)
    means[:k * c] = up(prev).reshape(-1)
    sums_d, counts_d = up(sums), up(counts)                           # (named: they must outlive the launch)
    ok(lib().vqseg_kmeans_finalize_f32(ptr(sums_d), ptr(counts_d), ptr(means), c, k, stream()))
    T.check_finalize(down(means, k * c, label), prev, sums, counts, label)


@pytest.mark.parametrize("n,c,k", [(1, 4, 1), (1025, 132, 3), (5 * 1024 + 77, 68, 64)])
def test_kmeans_accumulate_is_assign_then_code_sums(n, c, k):
    """vqseg_kmeans_accumulate_f32(samples, means) gives the bits and counts of vqseg_vq_code_sums(samples, vqseg_vq_assign_f32(samples,
    means)) -- and those pass every check of the constructed cases on the idx the assignment chose (K = 3 over 1025 rows: clusters of
    several segments at three channel groups)."""
    L = lib()
    x = T.dense_rows(6000 + n, n, c, False)
    means = x[np.random.RandomState(6001 + n).permutation(n)[:k]].copy()
    xd, md = up(x), up(means)
    label = f"accumulate ({n}, {c}, {k})"
    nbytes = L.vqseg_kmeans_workspace_bytes(n, c, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    sums, counts = out(k * c, F32), out(k, torch.int64)
    ok(L.vqseg_kmeans_accumulate_f32(ptr(xd), ptr(md), n, c, k, ptr(sums), ptr(counts), ptr(ws), nbytes, stream()))
    sums, counts = down(sums, k * c, label).reshape(k, c), down(counts, k, label)
    abytes = L.vqseg_vq_workspace_bytes(n, c, k)
    aws = torch.empty(abytes, dtype=torch.uint8, device=dev())
    idx = out(n, torch.int64)
    ok(L.vqseg_vq_assign_f32(ptr(xd), ptr(md), None, n, c, k, ptr(idx), None, ptr(aws), abytes, stream()))
    idx_h = down(idx, n, label)
    assert idx_h.min() >= 0 and idx_h.max() < k
    sums2, counts2 = code_sums(xd, idx[:n].contiguous(), n, c, k, False, label)
    assert (T.f32_bits(sums) == T.f32_bits(sums2)).all() and (counts == counts2).all()
    T.check_code_sums(sums, counts, x, idx_h, k, label)


# ---------------------------------------------------------------------------------------------------------------------
# 4. EMA
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,c,decay,eps", T.EMA_CASES)
def test_ema_update(k, c, decay, eps):
    """vqseg_vq_ema_update_f32 (ema_counts_kernel: K below, at and above its 256 threads; ema_embed_kernel: C below, at and above one and
    two 256-channel workgroups), decay 0 / 0.8 / 1, eps 1e-5 with empty codes (moving counts of 0 and 0.01 among them) and eps 0 with
    every code populated.  decay = 1 keeps cluster_size and embed_avg bit for bit, decay = 0 makes them float(counts) and sums bit for bit;
    everything else against oracle.torch_ref.vq_ema_update in float64 within the roundings counted from the source (T.ema_reference),
    each asserted to be below the bars of tests/test_vq_gpu.py."""
    _, _, counts, sums, cs0, avg0 = T.ema_inputs(k, c, eps)
    label = f"K={k} C={c} decay={decay} eps={eps}"
    cs, avg, cb, total = out(k, F32), out(k * c, F32), out(k * c, F32), out(1, F32)
    cs[:k] = up(cs0)
    avg[:k * c] = up(avg0).reshape(-1)
    sums_d, counts_d = up(sums), up(counts)                           # (named: they must outlive the launch)
    ok(lib().vqseg_vq_ema_update_f32(ptr(cs), ptr(avg), ptr(cb), ptr(sums_d), ptr(counts_d), c, k, decay, eps, ptr(total), stream()))
    T.check_ema(k, c, decay, eps, down(cs, k, label), down(avg, k * c, label), down(cb, k * c, label), down(total, 1, label)[0], label)
