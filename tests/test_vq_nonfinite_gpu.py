"""Non-finite and overflowing rows / codebooks through every VQ assign entry point (csrc/vq_assign.hip: vq_assign_f32_kernel, and csrc/vq_filter.hip:
vq_filter_bf16_kernel -> vq_resolve_kernel -> vq_rescore_kernel for bf16 rows) and what consumes the indices (gather, backward,
histogram, k-means lists).  A bf16 autocast step that diverges hands such rows to the layer; the reference computes through them
(torch.cdist -> argmin, vector_quantizer/vq_img.py:167-168) and so must this path: every row gets the code and the distance bits of
the CPU chain oracle (oracle/vq_chain.c, pinned on these very inputs by tests/test_vq_nonfinite_cpu.py) -- in particular a code in
[0, K), since the index goes unchecked into W + idx * C.  The clean rows of the same call must not notice their neighbours.

Why these cases bite (from the kernels' code, not from a run: the unfixed kernels would read out of bounds on them):
  * a row with a NaN score in every sub-chunk left vq_resolve_kernel with m = +inf, no candidate and no key: idx = 2^32 - 1;
  * a row whose distances are all +inf (norm_overflow, dot_overflow, neg_inf on the signed base) never moved the exact kernel's
    holder off its start value: idx = 2^31 - 1;
  * with K % 32 != 0 (the (301, 20, 33) and (301, 40, 300) shapes) a padding code's distance is NaN for a row with a NaN / Inf
    (inf * 0) and the clamp made it 0: a code >= K could win;
  * a NaN |e_k|^2 was dropped by the fmaxf reduction of en_max: the filter ranked the other codes, the exact kernel gives that
    code distance 0 on every row (nan_code: filter-on against filter-off would differ).
The modes compared: the filter, the filter with every row forced through the re-score (vq_filter_force_all), the exact kernel."""
import numpy as np
import pytest
import torch

from tests import synth
from tests import vq_poison as P
from tests.test_vq_filter_gpu import assert_identical, both_paths, dev

pytestmark = pytest.mark.gpu

FILTER_SHAPES = [(1029, 64, 256), (1029, 64, 512)]             # off the 128-row tile and the 256-row resolve block; one / two 256-code chunks
EXACT_SHAPES = [((301, 20, 33), "f32"), ((301, 40, 300), "bf16")]   # shapes the filter does not serve (K % 32 != 0: padding codes)
F32_ENTRY_SHAPE = (1029, 64, 256)
sid = lambda s: "x".join(map(str, s)) if isinstance(s[0], int) else "x".join(map(str, s[0])) + "-" + s[1]


def in_range(idx, k, what):
    """assertion 1, before anything consumes idx"""
    assert idx.dtype == torch.int64, what
    lo, hi = int(idx.min()), int(idx.max())
    assert 0 <= lo and hi < k, f"{what}: code indices span [{lo}, {hi}], K = {k}"


def assign_modes(rows_dev, W_dev, filtered):
    """-> {mode: (idx, dmin)}; for shapes the filter serves: filter, force_all and exact; otherwise the one path there is"""
    from vq_seg_amd import _hip
    k = W_dev.shape[0]
    if not filtered:
        before = _hip.set_option("vq_filter_launches", 0)
        out = _hip.vq_assign(rows_dev, W_dev, want_dmin=True)
        torch.cuda.synchronize()
        assert _hip.set_option("vq_filter_launches", before) == 0
        in_range(out[0], k, "exact")
        return {"exact": out}
    f, e = both_paths(rows_dev, W_dev)
    assert f[3] == 1, "the bf16 entry point did not take the candidate filter"
    in_range(f[0], k, "filter")
    in_range(e[0], k, "exact")
    prev = _hip.set_option("vq_filter_force_all", 1)
    try:
        a = _hip.vq_assign(rows_dev, W_dev, want_dmin=True)
        torch.cuda.synchronize()
    finally:
        _hip.set_option("vq_filter_force_all", prev)
    in_range(a[0], k, "force_all")
    assert_identical(f, e, "filter vs exact")
    assert_identical(a, e, "force_all vs exact")
    return {"filter": f[:2], "force_all": a, "exact": e}


def assert_oracle(modes, rows, W, what):
    """assertion 2: idx and the bits of dmin equal the chain oracle's on every row, in every mode"""
    from oracle import vq_chain
    ref_i, ref_d = vq_chain.assign(rows.numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
    for mode, (idx, dmin) in modes.items():
        got_i, got_d = idx.cpu().numpy(), dmin.cpu().numpy()
        bad = np.nonzero(got_i != ref_i)[0]
        assert bad.size == 0, f"{what} [{mode}]: {bad.size} indices differ from the oracle, first row {bad[:1]}: {got_i[bad[:1]]} vs {ref_i[bad[:1]]}"
        assert np.array_equal(got_d.view(np.uint32), ref_d.view(np.uint32)), f"{what} [{mode}]: distance bits differ from the oracle"


def run_rows(shape, dtype, kind, base, filtered):
    n, c, k = shape
    rows0, W0 = P.base(base, n, c, k)
    if dtype == "bf16":
        rows0 = rows0.bfloat16().float()                          # the layer's bf16 activations: exact bf16 values
    rows, W, m = P.poison_rows(rows0, W0, kind)
    cast = (lambda t: t.to(dev()).bfloat16()) if dtype == "bf16" else (lambda t: t.to(dev()))
    if dtype == "bf16":
        back = rows.bfloat16().float()
        assert bool(((back == rows) | (back.isnan() & rows.isnan())).all()), "a poison value is not exact in bf16"
    Wd = W.to(dev())
    modes = assign_modes(cast(rows), Wd, filtered)
    assert_oracle(modes, rows, W, f"{kind}/{base}")
    # assertion 3, isolation: the clean rows against the same call with the poisoned rows replaced by clean ones
    clean = assign_modes(cast(rows0), Wd, filtered)
    keep = (~m).to(dev())
    for mode in modes:
        assert torch.equal(modes[mode][0][keep], clean[mode][0][keep]), f"{kind}/{base} [{mode}]: clean rows' indices moved"
        assert np.array_equal(P.bits(modes[mode][1][keep]), P.bits(clean[mode][1][keep])), f"{kind}/{base} [{mode}]: clean rows' distances moved"


@pytest.mark.parametrize("base", P.BASES)
@pytest.mark.parametrize("kind", P.ROW_POISONS)
@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=sid)
def test_poisoned_bf16_rows_through_the_filter(shape, kind, base):
    run_rows(shape, "bf16", kind, base, filtered=True)


@pytest.mark.parametrize("base", P.BASES)
@pytest.mark.parametrize("kind", P.ROW_POISONS)
@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=sid)
def test_poisoned_rows_on_shapes_the_filter_does_not_serve(shape, kind, base):
    run_rows(shape[0], shape[1], kind, base, filtered=False)


@pytest.mark.parametrize("base", P.BASES)
@pytest.mark.parametrize("kind", P.ROW_POISONS)
def test_poisoned_f32_rows_through_the_f32_entry(kind, base):
    run_rows(F32_ENTRY_SHAPE, "f32", kind, base, filtered=False)


@pytest.mark.parametrize("base", P.BASES)
@pytest.mark.parametrize("kind", P.CODE_POISONS)
@pytest.mark.parametrize("shape", FILTER_SHAPES, ids=sid)
def test_poisoned_codebook_with_clean_rows(shape, kind, base):
    """a code the filter has no error bound for (non-finite |e_k|^2) must make it step aside, not rank the others"""
    n, c, k = shape
    rows, W0 = P.base(base, n, c, k)
    rows = rows.bfloat16().float()
    W = P.poison_codebook(W0, kind)
    modes = assign_modes(rows.to(dev()).bfloat16(), W.to(dev()), filtered=True)
    assert_oracle(modes, rows, W, f"{kind}/{base}")


def group_outputs(rows, books, training, **options):
    from vq_seg_amd import _hip
    prev = {key: _hip.set_option(key, val) for key, val in options.items()}
    try:
        preps = [_hip.vq_prepare(w) for w in books]
        out = _hip.vq_forward_group(rows, books, preps, training, [1.0, 0.5, 0.25])
        torch.cuda.synchronize()
    finally:
        for key, val in prev.items():
            _hip.set_option(key, val)
    for (q, idx, loss, dead), w in zip(out, books):
        in_range(idx, w.shape[0], "grouped forward")
    return out


def assert_level_bits(a, b, what):
    for name, u, v in zip(("quant", "idx", "loss", "dead"), a, b):
        assert np.array_equal(P.bits(u), P.bits(v)), f"{what}: {name} differs"


@pytest.mark.parametrize("training", [False, True], ids=["eval", "training"])
def test_grouped_forward_with_one_poisoned_level(training):
    """assertion 4: three levels in one launch, NaNs in the middle one only.  The gated exact launch then serves ONE level of the
    group; all three equal the filter-off call, the two clean ones equal a fully clean call."""
    shapes = [(1029, 64, 256), (517, 128, 256), (261, 256, 256)]
    clean, books = [], []
    for i, (n, c, k) in enumerate(shapes):
        r, w = P.base("relu", n, c, k, seed=340 + 10 * i)
        clean.append(r.bfloat16().float())
        books.append(w.to(dev()))
    poisoned = list(clean)
    poisoned[1] = P.poison_rows(clean[1], books[1].cpu(), "nan_one")[0]
    to_dev = lambda rs: [r.to(dev()).bfloat16() for r in rs]
    got = group_outputs(to_dev(poisoned), books, training)
    exact = group_outputs(to_dev(poisoned), books, training, vq_bf16_filter=0)
    base = group_outputs(to_dev(clean), books, training)
    for lvl in range(3):
        assert_level_bits(got[lvl], exact[lvl], f"level {lvl} against the filter-off call")
    for lvl in (0, 2):
        assert_level_bits(got[lvl], base[lvl], f"clean level {lvl} against the clean call")


@pytest.mark.parametrize("kind", ["nan_one", "norm_overflow"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_forward_and_backward_downstream_of_poisoned_rows(dtype, kind):
    """assertion 5: what consumes idx -- gather, histogram, commitment loss, backward -- on (1029, 64, 256)"""
    from oracle import vq_chain
    from vq_seg_amd import _hip
    n, c, k = 1029, 64, 256
    cw = 0.25
    rows0, W0 = P.base("relu", n, c, k)
    if dtype == "bf16":
        rows0 = rows0.bfloat16().float()
    rows, W, m = P.poison_rows(rows0, W0, kind)
    cast = (lambda t: t.to(dev()).bfloat16()) if dtype == "bf16" else (lambda t: t.to(dev()))
    Wd, keep = W.to(dev()), (~m).to(dev())
    ref_i, _ = vq_chain.assign(rows.numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
    # eval: quant is the code row, bit for bit; dead codes by the bincount definition
    quant, idx, loss, dead = _hip.vq_forward(cast(rows), Wd, False, cw)
    torch.cuda.synchronize()
    in_range(idx, k, "eval forward")
    assert np.array_equal(idx.cpu().numpy(), ref_i)
    assert np.array_equal(P.bits(quant), P.bits(Wd[idx] if dtype == "f32" else Wd[idx].bfloat16()))
    cnt = torch.bincount(idx, minlength=k)
    assert float(dead) == float(100 * ((cnt == 0).sum() / k))
    # training: clean rows' quant and input gradient equal those of the clean-input call
    g = synth.uniform(77, (n, c), -1.0, 1.0)
    gloss = torch.ones(1, device=dev())

    def train(r):
        x = cast(r)
        q, i, l, d = _hip.vq_forward(x, Wd, True, cw)
        torch.cuda.synchronize()
        in_range(i, k, "training forward")
        if dtype == "bf16":
            gx = _hip.vq_backward_bf16(cast(g), gloss, x, i, Wd, cw)
        else:
            gx = _hip.vq_backward(cast(g), gloss, x, q, cw)
        torch.cuda.synchronize()
        return q, i, l, d, gx

    q_p, i_p, l_p, d_p, gx_p = train(rows)
    q_c, i_c, l_c, d_c, gx_c = train(rows0)
    assert np.array_equal(i_p.cpu().numpy(), ref_i)
    assert np.array_equal(P.bits(q_p[keep]), P.bits(q_c[keep])), "clean rows' quantised values moved"
    assert np.array_equal(P.bits(gx_p[keep]), P.bits(gx_c[keep])), "clean rows' input gradient moved"
    cnt = torch.bincount(i_p, minlength=k)
    assert float(d_p) == float(100 * ((cnt == 0).sum() / k))
    # commitment loss: non-finite exactly when its fp64 restatement over the same idx is, as an fp32 value (the loss is an fp32
    # scalar: 2^140 / (N C) is finite in fp64 and not representable in fp32)
    with np.errstate(all="ignore"):
        x64 = rows.double().numpy()
        ref_loss = np.float32(cw * np.mean((W.double().numpy()[i_p.cpu().numpy()] - x64) ** 2))
    assert bool(torch.isfinite(l_p).all()) == bool(np.isfinite(ref_loss)), f"loss {float(l_p)} against the fp64 restatement {ref_loss}"
    assert not np.isfinite(ref_loss), "the poison was meant to reach the loss"
    assert bool(torch.isfinite(l_c).all())


def test_kmeans_with_nan_samples():
    """assertion 6: k-means shares the assign kernel; its histogram and member lists index by idx"""
    from oracle import vq_chain
    from vq_seg_amd import _hip
    n, c, k = 1029, 20, 33
    rows0, W = P.base("relu", n, c, k)
    rows, W, _ = P.poison_rows(rows0, W, "nan_one")
    ref_i, _ = vq_chain.assign(rows.numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
    means, bins = _hip.kmeans(rows.to(dev()), W.clone().to(dev()), 1)
    torch.cuda.synchronize()
    assert int(bins.sum()) == n
    assert np.array_equal(bins.cpu().numpy(), np.bincount(ref_i, minlength=k))
