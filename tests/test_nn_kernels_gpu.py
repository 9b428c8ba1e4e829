"""Direct parity of the BatchNorm, pooling, resize, head, cast and split-3 kernels (csrc/nn_bn.hip, nn_spatial.hip,
nn_head.hip, nn_stem.hip) through the C ABI against plain float64 computations of the same operations on the CPU.  The
reference always sees the values the kernel receives (inputs are rounded to the kernel's element type first).

Metric.  Element-wise kernels are held to a per-element bound
    |got - ref| <= k * u * S  (+ half a bf16 ulp of ref when the kernel stores bf16)
with u = 2^-24 (the kernels compute in fp32), S the float64 sum of the absolute values of the terms that make the element
and k the number of fp32 roundings in the kernel's expression, counted from the source and written next to each check.
Exact operations (pool values and positions, casts, split / merge, one-contribution pool gradients) are compared bit for bit.
Reduced quantities (statistics, dgamma / dbeta, the head's weight gradient, the batch terms inside g_y) use the bar the
repository already uses for fp32-accumulated sums against fp64: 2e-5 of the tensor scale (test_wgrad3x3_fused_taps),
running statistics 1e-5 (test_conv_bn_act_forward_backward).  No tolerance here is fitted to the kernels' output.
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

from tests import synth

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                    # unit roundoff of fp32
SUM_BAR = 2e-5                    # fp32-accumulated sums against fp64, of the tensor scale (test_wgrad3x3_fused_taps)
RUN_BAR = 1e-5                    # running statistics (test_conv_bn_act_forward_backward)
F32, BF16 = torch.float32, torch.bfloat16


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def lib():
    from vq_seg_amd import _hip
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def ok(rc):
    assert rc == 0, lib().vqseg_last_error()


def nan_like(shape, dtype):
    """Output buffers start as NaN (bytes: 0xff), so an element the kernel never wrote fails its check."""
    if dtype in (F32, BF16):
        return torch.full(tuple(shape), float("nan"), dtype=dtype, device=dev())
    return torch.full(tuple(shape), -1 if dtype != torch.uint8 else 255, dtype=dtype, device=dev())


@contextlib.contextmanager
def option(key, value):
    L = lib()
    prev = L.vqseg_set_option(key.encode(), value)
    assert prev >= 0, key
    try:
        yield
    finally:
        L.vqseg_set_option(key.encode(), prev)


def half_ulp_bf16(v):
    """Half a bf16 ulp (8 significand bits) at magnitude |v|: 2^(floor(log2 |v|) - 8)."""
    _, e = torch.frexp(v.abs().double().clamp_min(2.0 ** -126))          # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 9)


def check(got, ref, S, k, dtype, what, extra=None):
    """|got - ref| <= k u S (+ extra) (+ half a bf16 ulp at the magnitude the fp32 result can reach)."""
    got = got.detach().double().cpu().reshape(ref.shape)
    bound = k * U * S.double()
    if extra is not None:
        bound = bound + extra
    if dtype == BF16:
        bound = bound + half_ulp_bf16(ref.abs() + bound)
    err = (got - ref).abs()
    bad = ~(err <= bound)                                               # NaN counts as a failure
    if bad.any():
        ratio = err.nan_to_num(float("inf")) / (bound + 1e-300)
        ratio[~bad] = 0.0
        i = int(ratio.reshape(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat index {i}: "
                             f"got {got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r} bound {bound.reshape(-1)[i].item():.3e}")


def check_sum(got, ref, what, bar=SUM_BAR, scale=None, extra=0.0):
    got = got.detach().double().cpu().reshape(ref.shape)
    scale = ref.abs().max().item() if scale is None else scale
    err = ((got - ref).abs() - extra).max().item()
    assert err <= bar * scale, f"{what}: max error {err:.3e} over {bar:g} x scale {scale:.3e}"


def rnd(t, dtype):
    """Round an fp32 CPU tensor to the kernel's element type; returns (device tensor, float64 view of the same values)."""
    q = t.to(dtype)
    return q.to(dev()), q.double()


# ------------------------------------------------------------------------------------------------------------------
# 1. vqseg_bn_finalize_f
# ------------------------------------------------------------------------------------------------------------------
FINALIZE_CASES = [
    # M, C, branch
    (700, 8, "22 slots of 32 rows, short last slot: bn_finalize_kernel alone (slots <= 128)"),
    (1, 8, "M = 1: the unbiased-variance guard"),
    (8192, 64, "128 slots: the threshold itself, still one level"),
    (129 * 64 - 10, 64, "129 slots: two-level merge, last group a single short slot (no low parts)"),
    (200 * 64 - 3, 72, "200 slots, groups of 16, ragged last group of 8; ragged 64-channel group"),
    (2101 * 64 - 59, 64, "2101 slots, groups of 17, last group of 10: the unrolled level-2 fold and its tail"),
    (32 * 256 * 256, 64, "32768 slots (bench scale): groups of 256"),
    (4096, 1024, "C = 1024, one level"),
    (129 * 64, 1024, "C = 1024, two levels"),
]


def _finalize_partials(m, c, seed):
    """[slots, 2, C] (mean, M2) per slot, in fp64, of an [M, C] matrix whose channels have a mean of up to 1e3 standard
    deviations (the cancellation case).  Matrices above 4 M elements are not materialised: the slot statistics are drawn
    directly with the same spread (the kernel only ever sees the partials)."""
    rps = 64 if c >= 64 else 32
    n_slots = (m + rps - 1) // rps
    sd = 0.5 + 1.5 * synth.uniform(seed, (c,)).double()
    mu = sd * 1e3 * (2 * synth.uniform(seed + 1, (c,)).double() - 1) ** 3
    ns = torch.full((n_slots,), float(rps), dtype=torch.float64)
    ns[-1] = m - (n_slots - 1) * rps
    if m * c <= 4 << 20:
        x = mu + sd * math.sqrt(3.0) * synth.uniform(seed + 2, (m, c), -1, 1).double()
        x = torch.cat([x, torch.zeros(n_slots * rps - m, c, dtype=torch.float64)]).reshape(n_slots, rps, c)
        w = (torch.arange(rps)[None, :] < ns[:, None]).double()[..., None]
        mean = (x * w).sum(1) / ns[:, None]
        m2 = (((x - mean[:, None]) ** 2) * w).sum(1)
    else:
        mean = mu + sd * synth.uniform(seed + 2, (n_slots, c), -1, 1).double() / math.sqrt(rps) * 2
        m2 = sd ** 2 * ns[:, None] * (0.5 + synth.uniform(seed + 3, (n_slots, c)).double())
    return torch.stack([mean, m2], 1).float(), ns


@pytest.mark.parametrize("m,c,branch", FINALIZE_CASES, ids=[f"M{m}-C{c}" for m, c, _ in FINALIZE_CASES])
def test_bn_finalize_training(m, c, branch):
    L = lib()
    part, ns = _finalize_partials(m, c, 1000 + c + m % 977)
    slots_alloc = L.vqseg_conv_stat_slots(m, c)
    assert slots_alloc >= part.shape[0]
    gamma, beta = synth.uniform(11, (c,), 0.5, 1.5), synth.uniform(12, (c,), -0.5, 0.5)
    rm0, rv0 = synth.uniform(13, (c,), -1, 1), synth.uniform(14, (c,), 0.5, 1.5)
    mom, eps = 0.1, 1e-5
    momf = torch.tensor(mom, dtype=F32).double().item()                  # the float the kernel receives
    epsf = torch.tensor(eps, dtype=F32).double().item()
    # reference: Chan's merge of the SAME fp32 partials in float64
    p = part.double()
    mean = (ns[:, None] * p[:, 0]).sum(0) / m
    m2 = (p[:, 1] + ns[:, None] * (p[:, 0] - mean) ** 2).sum(0)
    var = m2 / m
    invstd = 1 / torch.sqrt(var + epsf)
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    unbiased = m2 / (m - 1) if m > 1 else var
    run_mean = (1 - momf) * rm0.double() + momf * mean
    run_var = (1 - momf) * rv0.double() + momf * unbiased
    for use_sync in (False, True):
        pd = torch.zeros((slots_alloc, 2, c), dtype=F32, device=dev())
        pd[:part.shape[0]] = part.to(dev())
        g, b, rm, rv = (t.to(dev()) for t in (gamma, beta, rm0.clone(), rv0.clone()))
        out = nan_like((4, c), F32)
        nbt = torch.full((1,), 5, dtype=torch.int64, device=dev())
        sync = torch.zeros(L.vqseg_bn_sync_ints(c), dtype=torch.int32, device=dev()) if use_sync else None
        ok(L.vqseg_bn_finalize_f(pd.data_ptr(), m, c, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), mom, eps, 1,
                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), nbt.data_ptr(), ptr(sync), stream()))
        torch.cuda.synchronize()
        tag = f"{branch} sync={use_sync}"
        o = out.double().cpu()
        # reduced quantities, per channel: 2e-5 of the terms that make them
        assert ((o[2] - mean).abs() <= SUM_BAR * mean.abs() + 1e-30).all(), f"save_mean {tag}"
        assert ((o[3] - invstd).abs() <= SUM_BAR * invstd).all(), f"save_invstd {tag}: {((o[3] - invstd).abs() / invstd).max():.3e}"
        assert ((o[0] - scale).abs() <= SUM_BAR * scale.abs()).all(), f"scale {tag}"
        assert ((o[1] - shift).abs() <= SUM_BAR * (beta.double().abs() + (mean * scale).abs())).all(), f"shift {tag}"
        assert ((rm.double().cpu() - run_mean).abs() <= RUN_BAR * ((1 - momf) * rm0.double().abs() + momf * mean.abs())).all(), f"run_mean {tag}"
        assert ((rv.double().cpu() - run_var).abs() <= RUN_BAR * run_var).all(), f"run_var {tag}"
        assert torch.isfinite(rv).all()
        assert nbt.item() == 6, tag
        if use_sync:
            assert not sync.any(), "the sync counters must read back as zeros"


@pytest.mark.parametrize("c", [8, 72, 1024])
def test_bn_finalize_eval(c):
    """Eval mode: coefficients from the running statistics in fp32, nothing updated.
    invstd = 1 / sqrtf(var + eps): 3 roundings; scale = gamma * invstd: 4; shift = beta - mean * scale: 6 on |beta| + |mean scale|."""
    L = lib()
    gamma, beta = synth.uniform(21, (c,), 0.5, 1.5), synth.uniform(22, (c,), -0.5, 0.5)
    rm0, rv0 = synth.uniform(23, (c,), -1, 1), synth.uniform(24, (c,), 0.01, 1.5)
    eps = 1e-5
    epsf = torch.tensor(eps, dtype=F32).double().item()
    g, b, rm, rv = (t.to(dev()) for t in (gamma, beta, rm0.clone(), rv0.clone()))
    out = nan_like((4, c), F32)
    nbt = torch.full((1,), 5, dtype=torch.int64, device=dev())
    ok(L.vqseg_bn_finalize_f(None, 77, c, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, eps, 0,
                             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), nbt.data_ptr(), None, stream()))
    torch.cuda.synchronize()
    invstd = 1 / torch.sqrt(rv0.double() + epsf)
    scale = gamma.double() * invstd
    check(out[3], invstd, invstd, 3, F32, "eval invstd")
    check(out[0], scale, scale.abs(), 4, F32, "eval scale")
    check(out[1], beta.double() - rm0.double() * scale, beta.double().abs() + (rm0.double() * scale).abs(), 6, F32, "eval shift")
    assert torch.equal(out[2].cpu(), rm0) and torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0) and nbt.item() == 5


# ------------------------------------------------------------------------------------------------------------------
# 2. vqseg_bn_apply_f / vqseg_bn_apply_bits_f
# ------------------------------------------------------------------------------------------------------------------
APPLY_CASES = [
    # M, C, wrap, branch
    (700, 64, False, "16-byte vectors, channel offset invariant under the grid stride (256 V % C == 0)"),
    (333, 72, False, "16-byte vectors, channel offset recomputed per trip"),
    (257, 13, False, "C % 8 != 0 and C % 4 != 0: the scalar path"),
    (8209, 128, True, "grid wrap: > 256 * 256 vectors under nn_grid_cap = 256"),
    (6007, 13, True, "grid wrap on the scalar path"),
]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("m,c,wrap,branch", APPLY_CASES, ids=[f"M{m}-C{c}" for m, c, _, _ in APPLY_CASES])
def test_bn_apply(m, c, wrap, branch, dtype):
    """out = relu?(fma(y, scale, shift) (+ res)): mul, add (fused on the vector paths: 1, spelled out on the scalar path: 2) and
    the residual add -> k = 2 without, 3 with a residual, on S = |y scale| + |shift| + |res|."""
    L = lib()
    yd, y = rnd(synth.uniform(31, (m, c), -2, 2), dtype)
    rd, r = rnd(synth.uniform(32, (m, c), -2, 2), dtype)
    sc, sh = synth.uniform(33, (c,), -1.5, 1.5), synth.uniform(34, (c,), -1, 1)
    scd, shd = sc.to(dev()), sh.to(dev())
    pre0 = y * sc.double() + sh.double()
    s0 = (y * sc.double()).abs() + sh.double().abs()
    for has_res in (False, True):
        pre = pre0 + r if has_res else pre0
        S = s0 + r.abs() if has_res else s0
        for relu in (0, 1):
            ref = pre.clamp_min(0) if relu else pre
            outs = []
            for cap in ((None, 256) if wrap else (None,)):
                out = nan_like((m, c), dtype)
                with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
                    ok(L.vqseg_bn_apply_f(int(dtype == BF16), yd.data_ptr(), ptr(rd) if has_res else None, scd.data_ptr(), shd.data_ptr(),
                                          m, c, relu, out.data_ptr(), stream()))
                torch.cuda.synchronize()
                check(out, ref, S, 3 if has_res else 2, dtype, f"bn_apply res={has_res} relu={relu} cap={cap} ({branch})")
                outs.append(out)
            if wrap:
                assert torch.equal(outs[0], outs[1]), "capped grid differs from the uncapped one"
            if relu and dtype == BF16 and c % 8 == 0:              # the bit-field form: same values, bits = (out > 0)
                for cap in ((None, 256) if wrap else (None,)):
                    out2 = nan_like((m, c), dtype)
                    bits = torch.zeros(m * c // 8, dtype=torch.uint8, device=dev())
                    with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
                        ok(L.vqseg_bn_apply_bits_f(yd.data_ptr(), ptr(rd) if has_res else None, scd.data_ptr(), shd.data_ptr(), m, c,
                                                   out2.data_ptr(), bits.data_ptr(), stream()))
                    torch.cuda.synchronize()
                    assert torch.equal(out2, outs[0])
                    assert torch.equal(bits.cpu(), _pack_bits(outs[0].cpu().float() > 0))
    if c % 8:
        out = nan_like((m, c), BF16)
        bits = torch.zeros(m * c // 8 + 1, dtype=torch.uint8, device=dev())
        assert L.vqseg_bn_apply_bits_f(yd.data_ptr(), None, scd.data_ptr(), shd.data_ptr(), m, c, out.data_ptr(), bits.data_ptr(), stream()) == -1


def _pack_bits(mask):
    """bit (i % 8) of byte i / 8 = mask.flat[i]"""
    b = mask.reshape(-1, 8).to(torch.int32)
    return (b << torch.arange(8, dtype=torch.int32)).sum(1).to(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------
# 3. vqseg_bn_backward_f / vqseg_bn_backward_bits_f
# ------------------------------------------------------------------------------------------------------------------
BWD_CASES = [
    # M, C, full cross of the variants, branch
    (700, 64, True, "ragged last row block"),
    (700, 13, True, "scalar path (C % 4 != 0)"),
    (131077, 72, False, "M >= 131073: rows per block double under sync; ragged channel group"),
    (300, 1024, False, "C = 1024: 16 channel groups"),
]
MARGIN = 0.05                     # |pre-activation| chosen at least this far from zero


def _bwd_variants(full, dtype, c):
    forms = ["none", "out", "recompute"] + (["bits"] if dtype == BF16 and c % 8 == 0 else [])
    for form in forms:
        for training in (1, 0):
            for use_sync in (False, True):
                for acc in ((0, 1) if full else (int(use_sync) ^ training,)):
                    for with_res in ((False, True) if form != "recompute" else (False,)):
                        if not full and with_res != bool(acc) and form != "recompute":
                            continue
                        for premask in ((1, 0) if form in ("out", "bits") and with_res else (1,)):
                            yield form, training, use_sync, acc, with_res, premask


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("m,c,full,branch", BWD_CASES, ids=[f"M{m}-C{c}" for m, c, _, _ in BWD_CASES])
def test_bn_backward(m, c, full, branch, dtype):
    """gz = g_out * mask; dbeta = sum gz, dgamma = sum gz xhat (2e-5 of the tensor scale, accumulate: onto nonzero values);
    g_res = gz exactly; g_y = k0 (gz - k1 - xhat k2), k0 = gamma invstd, k1 = dbeta / M, k2 = dgamma / M (eval: k0 gz).
    Roundings of g_y: y - mean, * invstd, * k2, gz - k1, - (xhat k2), * k0, and k0 / k1 / k2 themselves rounded to fp32: k = 8 on
    S = |k0| (|gz| + |k1| + |xhat k2|); the batch terms k1, k2 are reduced quantities and add |k0| 2e-5 (scale(k1) + |xhat| scale(k2))."""
    L = lib()
    bf = int(dtype == BF16)
    fsc = synth.uniform(41, (c,), 0.5, 1.5) * torch.where(synth.uniform(42, (c,)) < 0.25, -1.0, 1.0)
    fsh = synth.uniform(43, (c,), -1, 1)
    # the pre-activation first, away from zero; y derived from it and rounded to T
    u = synth.uniform(44, (m, c), -1, 1).double()
    pre_wanted = torch.sign(u) * (MARGIN + 2.0 * u.abs())
    yd, y = rnd(((pre_wanted - fsh.double()) / fsc.double()).float(), dtype)
    pre = y * fsc.double() + fsh.double()
    # condition of the recomputed mask: no element within 4x the worst-case fp32 evaluation error (2 roundings on |y s| + |shift|) of zero
    assert (pre.abs() > 4 * 2 * U * ((y * fsc.double()).abs() + fsh.double().abs())).all() and (pre != 0).all()
    mask = pre > 0
    outd, _ = rnd(pre.clamp_min(0).float(), dtype)
    assert torch.equal(outd.cpu().float() > 0, mask)
    bits = _pack_bits(mask).to(dev()) if c % 8 == 0 else None
    gd, g = rnd(synth.uniform(45, (m, c), -0.5, 1.0), dtype)
    mean, invstd = synth.uniform(46, (c,), -1, 1), synth.uniform(47, (c,), 0.5, 2)
    gamma = synth.uniform(48, (c,), 0.5, 1.5)
    dg0, db0 = synth.uniform(49, (c,), -3, 3), synth.uniform(50, (c,), -3, 3)
    meand, invstdd, gammad, fscd, fshd = (t.to(dev()) for t in (mean, invstd, gamma, fsc, fsh))
    xhat = (y - mean.double()) * invstd.double()
    k0 = gamma.double() * invstd.double()
    refs = {}
    for masked in (False, True):
        gz = g * mask if masked else g
        dbeta, dgamma = gz.sum(0), (gz * xhat).sum(0)
        refs[masked] = (gz, dbeta, dgamma)
    ws = torch.empty(L.vqseg_bn_backward_workspace_floats(m, c), dtype=F32, device=dev())
    n_run = 0
    for form, training, use_sync, acc, with_res, premask in _bwd_variants(full, dtype, c):
        gz, dbeta, dgamma = refs[form != "none"]
        k1, k2 = (dbeta / m, dgamma / m) if training else (torch.zeros(c, dtype=torch.float64),) * 2
        gy_ref = k0 * (gz - k1 - xhat * k2)
        S = k0.abs() * (gz.abs() + k1.abs() + (xhat * k2).abs())
        extra = k0.abs() * SUM_BAR * (k1.abs().max() + xhat.abs() * k2.abs().max())
        dgam, dbet = dg0.to(dev()), db0.to(dev())
        gy, gres = nan_like((m, c), dtype), (nan_like((m, c), dtype) if with_res else None)
        sync = torch.zeros(L.vqseg_bn_sync_ints(c), dtype=torch.int32, device=dev()) if use_sync else None
        ws.fill_(float("nan"))
        tag = f"form={form} training={training} sync={use_sync} accumulate={acc} g_res={with_res} premask={premask} ({branch})"
        with option("bn_bwd_premask", premask):
            if form == "bits":
                rc = L.vqseg_bn_backward_bits_f(gd.data_ptr(), bits.data_ptr(), yd.data_ptr(), meand.data_ptr(), invstdd.data_ptr(), gammad.data_ptr(),
                                                m, c, training, acc, ws.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), gy.data_ptr(), ptr(gres), ptr(sync), stream())
            else:
                rc = L.vqseg_bn_backward_f(bf, gd.data_ptr(), outd.data_ptr() if form == "out" else None, yd.data_ptr(), meand.data_ptr(), invstdd.data_ptr(),
                                           gammad.data_ptr(), fscd.data_ptr(), fshd.data_ptr(), m, c, int(form != "none"), training, acc, ws.data_ptr(),
                                           dgam.data_ptr(), dbet.data_ptr(), gy.data_ptr(), ptr(gres), ptr(sync), stream())
        assert rc == 0, (tag, L.vqseg_last_error())
        torch.cuda.synchronize()
        n_run += 1
        # accumulate: the sum is rounded to fp32 and added in fp32 (one more rounding, on the result)
        for name, got, ref0, add in (("dbeta", dbet, dbeta, db0), ("dgamma", dgam, dgamma, dg0)):
            ref = ref0 + add.double() if acc else ref0
            check_sum(got, ref, f"{name} {tag}", scale=ref0.abs().max().item(), extra=(2 * U * ref.abs()) if acc else 0.0)
        check(gy, gy_ref, S, 8, dtype, f"g_y {tag}", extra=extra)
        if with_res:
            assert torch.equal(gres.cpu().double(), gz), f"g_res {tag}"
        if use_sync:
            assert not sync.any(), f"sync counters not zero after {tag}"
    assert n_run >= 8
    # rejected arguments: return code only
    assert L.vqseg_bn_backward_f(bf, gd.data_ptr(), None, yd.data_ptr(), meand.data_ptr(), invstdd.data_ptr(), gammad.data_ptr(), None, None, m, c, 1, 1, 0,
                                 ws.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), gy.data_ptr(), None, None, stream()) == -1
    assert L.vqseg_bn_backward_f(bf, gd.data_ptr(), None, yd.data_ptr(), meand.data_ptr(), invstdd.data_ptr(), gammad.data_ptr(), None, None, 0, c, 0, 1, 0,
                                 ws.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), gy.data_ptr(), None, None, stream()) == -1


# ------------------------------------------------------------------------------------------------------------------
# 4. max-pool 3x3 / stride 2 / pad 1
# ------------------------------------------------------------------------------------------------------------------
def _pool_data(kind, seed, shape):
    n, h, w, c = shape
    if kind == "relu70":                                               # post-ReLU stem output: ~70 % zeros
        return synth.relu_features(seed, shape, sparsity=0.7)
    if kind == "grid8":                                                # eight levels: ties everywhere
        return torch.floor(synth.uniform(seed, shape) * 8) / 8 - 0.5
    if kind == "flat":                                                 # 4 x 4 patches of one value: windows that are entirely equal
        low = synth.uniform(seed, (n, (h + 3) // 4, (w + 3) // 4, c), -1, 1)
        return low.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w].contiguous()
    if kind == "negative":                                             # padding must never win
        return -(synth.uniform(seed, shape) + 0.125)
    raise ValueError(kind)


def _pool_case(L, dtype, n, h, w, c, kind, caps=(None,)):
    bf = int(dtype == BF16)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xd, x = rnd(_pool_data(kind, 60 + h + c, (n, h, w, c)), dtype)
    gd, g = rnd(synth.uniform(61, (n, ho, wo, c), -1, 1), dtype)
    ad, a = rnd(synth.uniform(62, (n, h, w, c), -1, 1), dtype)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr, ir = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    (gx_ref,) = torch.autograd.grad(yr, xr, g.permute(0, 3, 1, 2), retain_graph=True)
    gx_ref = gx_ref.permute(0, 2, 3, 1)
    # S = sum of |contributions|, cnt = their number, per input position
    (S,) = torch.autograd.grad(yr, xr, g.abs().permute(0, 3, 1, 2), retain_graph=True)
    (cnt,) = torch.autograd.grad(yr, xr, torch.ones_like(yr))
    S, cnt = S.permute(0, 2, 3, 1), cnt.permute(0, 2, 3, 1)
    ih, iw = ir // w, ir % w                                           # flat (ih * W + iw) -> window position kh * 3 + kw
    oh = torch.arange(ho).reshape(1, 1, ho, 1)
    ow = torch.arange(wo).reshape(1, 1, 1, wo)
    pos_ref = ((ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1))).permute(0, 2, 3, 1).to(torch.uint8)
    results = []
    for cap in caps:
        with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
            tag = f"{dtype} n={n} h={h} w={w} c={c} {kind} cap={cap}"
            y, idx = nan_like((n, ho, wo, c), dtype), nan_like((n, ho, wo, c), torch.uint8)
            ok(L.vqseg_maxpool3x3s2_f(bf, 0, xd.data_ptr(), None, n, h, w, c, y.data_ptr(), idx.data_ptr(), stream()))
            y2 = nan_like((n, ho, wo, c), dtype)
            ok(L.vqseg_maxpool3x3s2_f(bf, 0, xd.data_ptr(), None, n, h, w, c, y2.data_ptr(), None, stream()))
            torch.cuda.synchronize()
            assert torch.equal(y.cpu().double(), yr.detach().permute(0, 2, 3, 1)) and torch.equal(y2, y), f"pool values {tag}"
            assert torch.equal(idx.cpu(), pos_ref), f"pool positions (first maximum in scan order) {tag}"
            gx_x, gx_i, gx_a0, gx_a = (nan_like((n, h, w, c), dtype) for _ in range(4))
            ok(L.vqseg_maxpool3x3s2_f(bf, 1, xd.data_ptr(), gd.data_ptr(), n, h, w, c, gx_x.data_ptr(), None, stream()))
            ok(L.vqseg_maxpool3x3s2_f(bf, 1, None, gd.data_ptr(), n, h, w, c, gx_i.data_ptr(), idx.data_ptr(), stream()))
            ok(L.vqseg_maxpool3x3s2_backward_add_f(bf, gd.data_ptr(), idx.data_ptr(), None, n, h, w, c, gx_a0.data_ptr(), stream()))
            ok(L.vqseg_maxpool3x3s2_backward_add_f(bf, gd.data_ptr(), idx.data_ptr(), ad.data_ptr(), n, h, w, c, gx_a.data_ptr(), stream()))
            torch.cuda.synchronize()
            one = cnt <= 1
            for name, got in (("from x", gx_x), ("from idx, x = NULL", gx_i), ("add form, no addend", gx_a0)):
                # up to four contributions added in fp32: k = 3 on S; a single contribution is copied: exact
                check(got, gx_ref, S, 3, dtype, f"pool backward {name} {tag}")
                assert torch.equal(got.cpu().double()[one], gx_ref[one]), f"pool backward {name}: single contributions must be exact {tag}"
            # add form: the pooled gradient is rounded to T first (half a bf16 ulp of it), then one fp32 add and the store
            extra = half_ulp_bf16(gx_ref.abs() + 3 * U * S) * (~one) if dtype == BF16 else None
            check(gx_a, gx_ref + a, S + a.abs(), 4, dtype, f"pool backward add {tag}", extra=extra)
            results.append((y, idx, gx_x, gx_i, gx_a))
    return results


POOL_HW = [(18, 22), (17, 13), (2, 2), (1, 5)]


@pytest.mark.parametrize("kind", ["relu70", "grid8", "flat", "negative"])
@pytest.mark.parametrize("c", [64, 20, 3], ids=["C64-vec8or4", "C20-vec4orScalar", "C3-scalar"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_maxpool(dtype, c, kind):
    L = lib()
    for h, w in POOL_HW:
        _pool_case(L, dtype, 2, h, w, c, kind)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_maxpool_grid_stride(dtype):
    """> 256 * 256 work items with nn_grid_cap = 256: several trips per thread, bit-identical to the uncapped launch."""
    a, b = _pool_case(lib(), dtype, 2, 192, 200, 64, "relu70", caps=(None, 256))
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    a, b = _pool_case(lib(), dtype, 1, 300, 301, 3, "grid8", caps=(None, 256))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_maxpool_rejects_empty_shapes():
    L = lib()
    t = torch.zeros(64, device=dev())
    for n, h, w, c in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, -1, 4), (1, 4, 4, 0)):
        assert L.vqseg_maxpool3x3s2_f(0, 0, t.data_ptr(), None, n, h, w, c, t.data_ptr(), None, stream()) == -1
        assert L.vqseg_maxpool3x3s2_f(0, 1, t.data_ptr(), t.data_ptr(), n, h, w, c, t.data_ptr(), None, stream()) == -1
        assert L.vqseg_s3_maxpool3x3s2_f(t.data_ptr(), n, h, w, 8 if c > 0 else c, t.data_ptr(), stream()) == -1
        assert L.vqseg_bilinear_f(0, 0, t.data_ptr(), n, h, w, c, 2, 2, 0, t.data_ptr(), stream()) == -1


# ------------------------------------------------------------------------------------------------------------------
# 5. bilinear resize
# ------------------------------------------------------------------------------------------------------------------
def _axis(n_in, n_out, align):
    """Taps, weight and the fp32 error of the source coordinate of every output position (ATen's upsample_bilinear2d).
    The kernel evaluates s in fp32 -- a division, a multiplication, a subtraction, then s - floor(s): <= 4 u (|s| + 1) absolute."""
    d = torch.arange(n_out, dtype=torch.float64)
    if align:
        s = d * ((n_in - 1) / (n_out - 1)) if n_out > 1 else torch.zeros(n_out, dtype=torch.float64)
    else:
        s = ((d + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0, 4 * U * (s + 1)


def _near(i0, n_in):
    return [(i0 + j).clamp(0, n_in - 1) for j in (-1, 0, 1, 2)]


def _bilinear_refs(x, g, ho, wo, align):
    """fp64 forward / backward (torch) plus the bound terms.  x [n,h,w,c], g [n,ho,wo,c] (float64)."""
    n, h, w, c = x.shape
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    yr = F.interpolate(xr, size=(ho, wo), mode="bilinear", align_corners=bool(align))
    (gx,) = torch.autograd.grad(yr, xr, g.permute(0, 3, 1, 2), retain_graph=True)
    (Sb,) = torch.autograd.grad(yr, xr, g.abs().permute(0, 3, 1, 2))        # the weights are >= 0: sum |w g|
    y_ref, gx_ref, Sb = yr.detach().permute(0, 2, 3, 1), gx.permute(0, 2, 3, 1), Sb.permute(0, 2, 3, 1)
    h0, h1, lh, eh = _axis(h, ho, align)
    w0, w1, lw, ew = _axis(w, wo, align)
    lh_, lw_, eh_, ew_ = lh.reshape(1, ho, 1, 1), lw.reshape(1, 1, wo, 1), eh.reshape(1, ho, 1, 1), ew.reshape(1, 1, wo, 1)
    X = x.abs()

    def mix_w(t):                                                      # [n, *, w, c] -> [n, *, wo, c]
        return (1 - lw_) * t[:, :, w0] + lw_ * t[:, :, w1]

    def mix_h(t):
        return (1 - lh_) * t[:, h0] + lh_ * t[:, h1]

    own = mix_h(mix_w(x))
    assert (own - y_ref).abs().max() <= 1e-12 * (1 + x.abs().max()), "the test's own taps disagree with F.interpolate"
    Sf = mix_h(mix_w(X))
    # a coordinate error e moves the result by at most e * (sum of |x| over the rows / columns around the taps)
    coord_f = eh_ * mix_w(sum(X[:, j] for j in _near(h0, h))) + ew_ * mix_h(sum(X[:, :, j] for j in _near(w0, w)))
    # backward: the same displacement on every contribution, scattered
    G = g.abs()

    def scat_w(t, near):                                               # [n, *, wo, c] -> [n, *, w, c]
        out = torch.zeros(t.shape[0], t.shape[1], w, c, dtype=torch.float64)
        if near:
            for j in _near(w0, w):
                out.index_add_(2, j, t)
        else:
            out.index_add_(2, w0, t * (1 - lw_))
            out.index_add_(2, w1, t * lw_)
        return out

    def scat_h(t, near):
        out = torch.zeros(t.shape[0], h, t.shape[2], c, dtype=torch.float64)
        if near:
            for j in _near(h0, h):
                out.index_add_(1, j, t)
        else:
            out.index_add_(1, h0, t * (1 - lh_))
            out.index_add_(1, h1, t * lh_)
        return out

    own_b = scat_h(scat_w(g, False), False)
    assert (own_b - gx_ref).abs().max() <= 1e-12 * (1 + g.abs().max()) * (1 + ho * wo / (h * w))
    coord_b = scat_h(scat_w(G * eh_, False), True) + scat_h(scat_w(G * ew_, True), False)
    return y_ref, Sf, coord_f, gx_ref, Sb, coord_b


RESIZE_CASES = [
    # h, w, ho, wo, branch
    (16, 32, 32, 64, "exact 2x, power-of-two extents: up2 forward, four-row backward"),
    (2, 4, 4, 8, "exact 2x with H = 2: up2 forward, one-row backward"),
    (1, 2, 2, 4, "exact 2x from a single row"),
    (9, 11, 18, 22, "exact 2x, extents not powers of two: generic kernels"),
    (18, 22, 35, 41, "ragged up-scale"),
    (7, 5, 30, 23, "ragged up-scale above 4x: the backward's search range"),
    (2, 2, 17, 17, "two rows to seventeen: (out-1)/(in-1) = 16 under align_corners"),
    (18, 22, 7, 9, "ragged down-scale"),
    (12, 10, 12, 10, "identity"),
    (1, 1, 5, 7, "input extents of 1"),
    (1, 6, 4, 6, "input height 1"),
    (5, 7, 1, 1, "output extents of 1 (align_corners: ho - 1 = 0)"),
    (6, 4, 1, 9, "output height 1"),
]


def _resize_case(L, dtype, n, c, h, w, ho, wo, align, caps=(None,), tag=""):
    bf = int(dtype == BF16)
    xd, x = rnd(synth.uniform(70 + c, (n, h, w, c), -1, 1), dtype)
    gd, g = rnd(synth.uniform(71 + c, (n, ho, wo, c), -1, 1), dtype)
    y_ref, Sf, coord_f, gx_ref, Sb, coord_b = _bilinear_refs(x, g, ho, wo, align)
    # forward: bil_mix is 1 - lw, (1 - lw) v00, fma per row pair, then 1 - lh, (1 - lh) top, fma: a chain of 7 roundings
    # backward: per contribution 1 - l (x2), wh * ww, the fma, and the fmas of the contributions after it; at most
    # (2 ceil(ho / h) + 2) (2 ceil(wo / w) + 2) contributions touch an input position
    kb = (2 * -(-ho // h) + 2) * (2 * -(-wo // w) + 2) + 3
    res = []
    for cap in caps:
        y, gx = nan_like((n, ho, wo, c), dtype), nan_like((n, h, w, c), dtype)
        with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
            ok(L.vqseg_bilinear_f(bf, 0, xd.data_ptr(), n, h, w, c, ho, wo, align, y.data_ptr(), stream()))
            ok(L.vqseg_bilinear_f(bf, 1, gd.data_ptr(), n, h, w, c, ho, wo, align, gx.data_ptr(), stream()))
        torch.cuda.synchronize()
        t = f"{dtype} c={c} {h}x{w} -> {ho}x{wo} align_corners={align} cap={cap} {tag}"
        check(y, y_ref, Sf, 7, dtype, f"bilinear forward {t}", extra=coord_f)
        check(gx, gx_ref, Sb, kb, dtype, f"bilinear backward {t}", extra=coord_b)
        res.append((y, gx))
    return res


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("h,w,ho,wo,branch", RESIZE_CASES, ids=[f"{a}x{b}-{p}x{q}" for a, b, p, q, _ in RESIZE_CASES])
def test_bilinear(h, w, ho, wo, branch, align):
    """C = 64 / 36 / 20 / 3 / 5: fp32 vectors of 4 (C = 36, 20: channel-vector counts that are not powers of two, so never the
    up2 kernels), the 3-class form, scalar; bf16 vectors of 8 (C = 64) and scalar."""
    L = lib()
    for dtype in (F32, BF16):
        for c in (64, 36, 20, 3, 5):
            _resize_case(L, dtype, 2, c, h, w, ho, wo, align, tag=branch)
    if ho == 2 * h and wo == 2 * w and not align:                      # the up2 kernels against their generic and one-row siblings
        for mode in (0, 2):
            with option("bilinear_up2", mode):
                for dtype in (F32, BF16):
                    _resize_case(L, dtype, 2, 64, h, w, ho, wo, align, tag=f"bilinear_up2={mode}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_bilinear_grid_stride(dtype):
    L = lib()
    for h, w, ho, wo, align in ((64, 64, 128, 128, 0), (60, 64, 100, 120, 0), (60, 64, 100, 120, 1), (150, 160, 64, 70, 0)):
        a, b = _resize_case(L, dtype, 3, 64, h, w, ho, wo, align, caps=(None, 256))
        assert all(torch.equal(p, q) for p, q in zip(a, b)), (h, w, ho, wo, align)


# ------------------------------------------------------------------------------------------------------------------
# 6. 1x1 head
# ------------------------------------------------------------------------------------------------------------------
def _split3(v):
    """fp32 [rows, C] -> split-3 rows [rows, 2C] bf16 = [hi | lo], hi = bf16(v), lo = bf16(v - hi)"""
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return torch.cat([hi, lo], -1)


def _merge3(s):
    c = s.shape[-1] // 2
    return s[..., :c].float() + s[..., c:].float()


@pytest.mark.parametrize("cin", [8, 24, 32, 64])
@pytest.mark.parametrize("m", [1, 2047, 2049, 70000])
def test_head1x1(m, cin):
    """Rows straddle HEAD_ROWS = 2048; Cin = 24 is the chunk count that does not divide the 256 threads of the weight kernel.
    forward: a chain of Cin fmas (k = Cin; split-3 rows: + 1 for hi + lo) on S = sum |x w|; data gradient: Cout fmas (k = Cout) on
    sum |g w|, add form + the add; weight gradient: a reduced quantity (2e-5 of the tensor scale)."""
    L = lib()
    for cout in (1, 3, 4):
        w = synth.uniform(80 + cout, (cout, cin), -1, 1)
        wd, w64 = w.to(dev()), w.double()
        gd, g = rnd(synth.uniform(81, (m, cout), -1, 1), F32)
        x0 = synth.uniform(82, (m, cin), -0.5, 1.0)
        ws = torch.empty(max(L.vqseg_head1x1_backward_workspace_floats(m, cin, cout), 1), dtype=F32, device=dev())
        for kind in (0, 1, 2):
            if kind == 2:
                rows = _split3(x0)
                xd, x = rows.to(dev()), rows[:, :cin].double() + rows[:, cin:].double()
            else:
                xd, x = rnd(x0, BF16 if kind else F32)
            t = f"row type {kind} m={m} cin={cin} cout={cout}"
            y = nan_like((m, cout), F32)
            ok(L.vqseg_head1x1_forward_f(kind, xd.data_ptr(), wd.data_ptr(), m, cin, cout, y.data_ptr(), stream()))
            torch.cuda.synchronize()
            check(y, x @ w64.T, x.abs() @ w64.abs().T, cin + (kind == 2), F32, f"head forward {t}")
            if kind == 2:
                continue
            dtype = BF16 if kind else F32
            ad, a = rnd(synth.uniform(83, (m, cin), -1, 1), dtype)
            gx_ref, Sx = g @ w64, g.abs() @ w64.abs()
            gw_ref = g.T @ x
            for add in (None, "null", "given"):
                gx, gw = nan_like((m, cin), dtype), nan_like((cout, cin), F32)
                ws.fill_(float("nan"))
                if add is None:
                    ok(L.vqseg_head1x1_backward_f(kind, xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), m, cin, cout, gx.data_ptr(), gw.data_ptr(),
                                                  ws.data_ptr(), stream()))
                else:
                    ok(L.vqseg_head1x1_backward_add_f(kind, xd.data_ptr(), wd.data_ptr(), gd.data_ptr(), m, cin, cout, gx.data_ptr(), gw.data_ptr(),
                                                      ws.data_ptr(), ad.data_ptr() if add == "given" else None, stream()))
                torch.cuda.synchronize()
                if add == "given":                                    # the data gradient rounded to T first, then one fp32 add
                    extra = half_ulp_bf16(gx_ref.abs() + cout * U * Sx) if kind else None
                    check(gx, gx_ref + a, Sx + a.abs(), cout + 1, dtype, f"head data gradient + addend {t}", extra=extra)
                else:
                    check(gx, gx_ref, Sx, cout, dtype, f"head data gradient {t} add={add}")
                check_sum(gw, gw_ref, f"head weight gradient {t} add={add}")
    bad_x = torch.zeros(64, device=dev())
    assert L.vqseg_head1x1_forward_f(0, bad_x.data_ptr(), bad_x.data_ptr(), 1, 12, 3, bad_x.data_ptr(), stream()) == -1     # Cin % 8
    assert L.vqseg_head1x1_forward_f(0, bad_x.data_ptr(), bad_x.data_ptr(), 1, 8, 5, bad_x.data_ptr(), stream()) == -1      # Cout > 4


# ------------------------------------------------------------------------------------------------------------------
# 7. casts and split-3 helpers
# ------------------------------------------------------------------------------------------------------------------
def _cast_values(n):
    v = synth.uniform(90, (n,), -4, 4)
    v[::7] *= 1e-3
    v[::11] *= 1e4
    # up to the next binade and ties to even; +-0 and subnormals; overflow to infinity and infinities
    raw = [0x3F7FFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x3F808000, 0x3F818000, 0x3F808001, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
           0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F800000, 0xFF800000, 0x0000C000, 0x00010000]
    special = torch.tensor([r - (1 << 32) if r >= (1 << 31) else r for r in raw], dtype=torch.int32).view(F32)
    v[:min(n, special.numel())] = special[:n]
    return v


@pytest.mark.parametrize("n,cap", [(1, None), (1000003, None), (1000003, 256)], ids=["one", "odd", "odd-grid-wrap"])
def test_cast(n, cap):
    """fp32 -> bf16 is round-to-nearest-even (torch's own conversion), bf16 -> fp32 is exact: bits.  Values that round up into the
    next binade, ties, +-0, subnormals, the largest finite values and infinities are among the inputs."""
    L = lib()
    v = _cast_values(max(n, 32))[:n]
    vd = v.to(dev())
    with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
        b = nan_like((n,), BF16)
        ok(L.vqseg_cast_f(1, vd.data_ptr(), n, b.data_ptr(), stream()))
        f = nan_like((n,), F32)
        ok(L.vqseg_cast_f(0, b.data_ptr(), n, f.data_ptr(), stream()))
    torch.cuda.synchronize()
    want = v.bfloat16()
    assert torch.equal(b.cpu().view(torch.int16), want.view(torch.int16)), "fp32 -> bf16 is not round-to-nearest-even"
    assert torch.equal(f.cpu().view(torch.int32), want.float().view(torch.int32)), "bf16 -> fp32 is not exact"
    assert L.vqseg_cast_f(1, vd.data_ptr(), 0, b.data_ptr(), stream()) == -1


@pytest.mark.parametrize("rows,c,cap", [(1001, 24, None), (1, 8, None), (9001, 64, None), (9001, 64, 256)],
                         ids=["odd-rows", "one-row", "tall", "tall-grid-wrap"])
def test_s3_split_merge(rows, c, cap):
    """hi = bf16(v), lo = bf16(v - hi); merge = hi + lo in fp32: both exact operations, compared bit for bit."""
    L = lib()
    v = _cast_values(rows * c).reshape(rows, c).clamp(-3e38, 3e38)
    v[v.abs() < 1e-30] = 0.0                                           # the split of fp32 subnormals is not part of the contract
    vd = v.to(dev())
    with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
        s = nan_like((rows, 2 * c), BF16)
        ok(L.vqseg_s3_split_f(vd.data_ptr(), rows, c, s.data_ptr(), stream()))
        mrg = nan_like((rows, c), F32)
        ok(L.vqseg_s3_merge_f(s.data_ptr(), rows, c, mrg.data_ptr(), stream()))
    torch.cuda.synchronize()
    want = _split3(v)
    assert torch.equal(s.cpu().view(torch.int16), want.view(torch.int16)), "split-3 rows differ from hi = bf16(v), lo = bf16(v - hi)"
    assert torch.equal(mrg.cpu().view(torch.int32), _merge3(want).view(torch.int32)), "merge differs from hi + lo"
    assert L.vqseg_s3_split_f(vd.data_ptr(), rows, 12, s.data_ptr(), stream()) == -1


@pytest.mark.parametrize("n,h,w,c,cap", [(2, 18, 22, 24, None), (2, 17, 13, 8, None), (1, 1, 5, 8, None), (2, 2, 2, 64, None),
                                         (2, 190, 200, 64, None), (2, 190, 200, 64, 256)])
def test_s3_maxpool(n, h, w, c, cap):
    """The pool of the merged values, re-split: exact."""
    L = lib()
    rows = _split3(_pool_data("relu70" if h % 2 == 0 else "grid8", 95, (n, h, w, c)) * 1.2345678)
    merged = _merge3(rows)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = nan_like((n, ho, wo, 2 * c), BF16)
    with option("nn_grid_cap", cap) if cap else contextlib.nullcontext():
        ok(L.vqseg_s3_maxpool3x3s2_f(rows.to(dev()).data_ptr(), n, h, w, c, y.data_ptr(), stream()))
    torch.cuda.synchronize()
    want = _split3(F.max_pool2d(merged.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous())
    assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("h,w,ho,wo,c,cap", [(16, 32, 32, 64, 64, None), (16, 32, 32, 64, 24, None), (9, 11, 18, 22, 8, None), (18, 22, 35, 41, 8, None),
                                             (7, 5, 30, 23, 8, None), (1, 1, 5, 7, 8, None), (5, 7, 1, 1, 8, None), (18, 22, 7, 9, 16, None),
                                             (64, 64, 128, 128, 64, 256), (60, 64, 100, 120, 64, 256)])
def test_s3_bilinear(h, w, ho, wo, c, cap, align):
    """The resize of the merged fp32 values (the forward bound of test_bilinear), re-split: hi + lo represents the fp32 result
    to 2^-17 of its magnitude (lo is the bf16 rounding of a remainder of at most 2^-9 |v|: 2^-9 2^-9 / 2 = 2^-19; 2^-17 allows for hi's ties)."""
    L = lib()
    n = 2
    rows = _split3(synth.uniform(97, (n, h, w, c), -1, 1))
    x = rows[..., :c].double() + rows[..., c:].double()
    y_ref, Sf, coord_f, _, _, _ = _bilinear_refs(x, torch.zeros(n, ho, wo, c, dtype=torch.float64), ho, wo, align)
    outs = []
    for cp in ((None, cap) if cap else (None,)):
        y = nan_like((n, ho, wo, 2 * c), BF16)
        with option("nn_grid_cap", cp) if cp else contextlib.nullcontext():
            ok(L.vqseg_s3_bilinear_f(rows.to(dev()).data_ptr(), n, h, w, c, ho, wo, align, y.data_ptr(), stream()))
        torch.cuda.synchronize()
        yc = y.cpu()
        check(yc[..., :c].double() + yc[..., c:].double(), y_ref, Sf, 7 + 1, F32, f"s3 bilinear cap={cp}", extra=coord_f + 2.0 ** -17 * y_ref.abs())
        outs.append(y)
    if cap:
        assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------------------------
# 8. the split-3 pool and resize are the fp32 kernels on other rows:  s3_op(r) == s3_split(f32_op(s3_merge(r))), bit for bit
# ------------------------------------------------------------------------------------------------------------------
def _s3_through_f32(L, rows, n, h, w, c, ho, wo, f32_op):
    """s3_split(f32_op(s3_merge(rows))) through the C ABI: the merge and the split are exact, so this is what the split-3 entry
    point must return if it evaluates the fp32 kernel's expressions on the same values in the same order."""
    merged = nan_like((n, h, w, c), F32)
    ok(L.vqseg_s3_merge_f(rows.data_ptr(), n * h * w, c, merged.data_ptr(), stream()))
    y32 = nan_like((n, ho, wo, c), F32)
    f32_op(merged, y32)
    want = nan_like((n, ho, wo, 2 * c), BF16)
    ok(L.vqseg_s3_split_f(y32.data_ptr(), n * ho * wo, c, want.data_ptr(), stream()))
    return want


@pytest.mark.parametrize("n,h,w,c", [(2, 17, 13, 8), (1, 1, 5, 8), (2, 18, 22, 24)],
                         ids=["odd-extents-one-vector", "single-row-clipped-windows", "cv3"])
def test_s3_maxpool_is_f32_maxpool(n, h, w, c):
    L = lib()
    rows = _split3(synth.uniform(98, (n, h, w, c), -1, 1)).to(dev())
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    got = nan_like((n, ho, wo, 2 * c), BF16)
    ok(L.vqseg_s3_maxpool3x3s2_f(rows.data_ptr(), n, h, w, c, got.data_ptr(), stream()))
    want = _s3_through_f32(L, rows, n, h, w, c, ho, wo, lambda x, y: ok(
        L.vqseg_maxpool3x3s2_f(0, 0, x.data_ptr(), None, n, h, w, c, y.data_ptr(), None, stream())))
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("h,w,ho,wo,c", [(16, 32, 32, 64, 64), (16, 32, 32, 64, 24), (9, 11, 18, 22, 8), (7, 5, 30, 23, 8), (5, 7, 1, 1, 8)],
                         ids=["exact2x", "generic-cv-not-pow2", "generic-2x-odd", "generic-up", "generic-to-1x1"])
def test_s3_bilinear_is_f32_bilinear(h, w, ho, wo, c, align):
    """16x32 -> 32x64 with C = 64 takes the exact-2x kernels on both sides for align = 0 (cv = 8 split-3, 16 fp32: powers of two);
    it runs again with bilinear_up2 = 0 (the generic kernels).  C = 24: cv = 3 / 6, never the exact-2x kernels."""
    L = lib()
    n = 2
    rows = _split3(synth.uniform(97, (n, h, w, c), -1, 1)).to(dev())
    exact2x = ho == 2 * h and wo == 2 * w and c == 64
    for up2 in ((None, 0) if exact2x else (None,)):
        with option("bilinear_up2", up2) if up2 is not None else contextlib.nullcontext():
            got = nan_like((n, ho, wo, 2 * c), BF16)
            ok(L.vqseg_s3_bilinear_f(rows.data_ptr(), n, h, w, c, ho, wo, align, got.data_ptr(), stream()))
            want = _s3_through_f32(L, rows, n, h, w, c, ho, wo, lambda x, y: ok(
                L.vqseg_bilinear_f(0, 0, x.data_ptr(), n, h, w, c, ho, wo, align, y.data_ptr(), stream())))
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"bilinear_up2={up2}"
