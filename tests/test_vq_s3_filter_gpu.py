"""Split-3 rows as a row type of the VQ launch path (csrc/vq_filter.hip, vq_assign.hip, vq_tail.hip; row type 2 of
vqseg_vq_forward_group, vqseg_vq_assign_s3).  A split-3 row is [hi | lo] bf16 and its logical value the fp32 sum hi + lo; every result
must be the exact kernel's on the merged rows: the comparison arm is vqseg_s3_merge_f followed by the exact fp32 kernel with the filters
off, and indices AND distance bits must be identical -- with the candidate filter on the [hi | lo] halves (the default), with every row
forced through the exact re-score (vq_filter_force_all = 1) and with the exact kernel merging on load (vq_s3_filter = 0).  The direct
[hi | lo] gather must write the bytes of the fp32 gather followed by vqseg_s3_split_f.
Reference arithmetic replaced: torch.cdist -> argmin -> embedding lookup of EuclideanCodebook.forward (vector_quantizer/vq_img.py:167-171)
on the fp32 features of the reference trainers' no-grad pseudo-label forwards."""
import ctypes

import numpy as np
import pytest
import torch

from tests import synth, vq_poison

pytestmark = pytest.mark.gpu

MODES = {"filter": {}, "force_all": {"vq_filter_force_all": 1}, "s3_exact": {"vq_s3_filter": 0}}


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def s3_split(x):
    """fp32 rows (N, C) on the GPU -> split-3 rows (N, 2C) bf16 (vqseg_s3_split_f)"""
    from vq_seg_amd import _hip
    n, c = x.shape
    y = torch.empty((n, 2 * c), dtype=torch.bfloat16, device=x.device)
    _hip.launch("vqseg_s3_split_f", x.device, _hip.tptr(x, "rows", dtype=torch.float32, numel=n * c), n, c, _hip.tptr(y, "split-3 rows", bf=2, numel=2 * n * c))
    return y


def s3_merge(y):
    from vq_seg_amd import _hip
    n, c2 = y.shape
    x = torch.empty((n, c2 // 2), dtype=torch.float32, device=y.device)
    _hip.launch("vqseg_s3_merge_f", y.device, _hip.tptr(y, "split-3 rows", bf=2, numel=n * c2), n, c2 // 2, _hip.tptr(x, "rows", dtype=torch.float32, numel=n * c2 // 2))
    return x


class options:
    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from vq_seg_amd import _hip
        self.prev = {k: _hip.set_option(k, v) for k, v in self.opts.items()}

    def __exit__(self, *exc):
        from vq_seg_amd import _hip
        for k, v in self.prev.items():
            _hip.set_option(k, v)
        return False


def bits32(t):
    return t.cpu().numpy().view(np.uint32)


def run_all_modes(rows, W, what, oracle_rows=1024):
    """rows (N, C), W (K, C) fp32 on the CPU.  -> {mode: (pairs, overflow flag, filter launches)} after asserting that every mode's
    indices and distance bits are those of the exact kernel on the merged rows and of the CPU chain oracle on a slice of them."""
    from oracle import vq_chain
    from vq_seg_amd import _hip
    s3 = s3_split(rows.to(dev()).contiguous())
    merged = s3_merge(s3)
    Wd = W.to(dev()).contiguous()
    with options(vq_bf16_filter=0, vq_s3_filter=0):
        idx_e, d_e = _hip.vq_assign(merged, Wd, want_dmin=True)
        torch.cuda.synchronize()
    sl = slice(0, min(oracle_rows, rows.shape[0]))
    ref_i, ref_d = vq_chain.assign(merged[sl].cpu().numpy(), W.numpy(), vq_chain.ORDER_MFMA8)
    assert np.array_equal(idx_e[sl].cpu().numpy(), ref_i), f"{what}: the comparison arm differs from the chain oracle"
    assert np.array_equal(bits32(d_e[sl]), ref_d.view(np.uint32)), f"{what}: the comparison arm's distance bits differ from the chain oracle"
    out = {}
    for mode, opts in MODES.items():
        with options(**opts):
            before = _hip.set_option("vq_filter_launches", 0)
            idx, d, state = _hip.vq_assign(s3, Wd, want_dmin=True, s3=True, want_filter_state=True)
            torch.cuda.synchronize()
            took = _hip.set_option("vq_filter_launches", before)
        assert torch.equal(idx, idx_e), f"{what} [{mode}]: {int((idx != idx_e).sum())} of {idx.numel()} indices differ from the exact kernel on the merged rows"
        assert np.array_equal(bits32(d), bits32(d_e)), f"{what} [{mode}]: distance bits differ"
        filtered = mode != "s3_exact" and _hip.lib().vqseg_vq_filter_counter_offset(rows.shape[0], rows.shape[1], W.shape[0]) != 0
        assert took == (1 if filtered else 0), f"{what} [{mode}]: {took} filter launches"
        st = state.cpu().numpy() if (filtered and state is not None) else None
        out[mode] = (None if st is None else int(st[:64].sum()), None if st is None else int(st[64]), took)
    print(f"{what}: N {rows.shape[0]} C {rows.shape[1]} K {W.shape[0]}: " + ", ".join(f"{m} pairs {v[0]} overflow {v[1]}" for m, v in out.items()))
    return out


def separated(seed, n, c, k):
    """a codebook of sparse post-ReLU codes and rows that are codes plus a tenth of their scale in noise: the nearest code is nearer by
    orders of magnitude more than the filter's band (2.4e-4 |x| |e| at C = 64)"""
    W = synth.relu_features(seed, (k, c), sparsity=0.3, scale=1.5)
    rows = W[(torch.arange(n) * 13 + 5) % k] + 0.1 * synth.uniform(seed + 1, (n, c), -1, 1)
    return rows, W


# (129, 32, 256): one stage, one chunk, ragged last tile; (3000, 64, 256): the adversarial suite's shape; (1000, 96, 512): two code
# chunks, odd stage count
@pytest.mark.parametrize("n,c,k", [(129, 32, 256), (3000, 64, 256), (1000, 96, 512)])
def test_s3_rows_equal_the_exact_kernel_on_the_merged_rows(n, c, k):
    rows, W = separated(400 + c, n, c, k)
    out = run_all_modes(rows, W, "separated")
    pairs, overflow, took = out["filter"]
    # against a vacuous pass: the filter ran, decided (no overflow into the exact kernel) and re-scored fewer pairs than its list holds
    assert took == 1 and overflow == 0 and pairs < 4 * n, (took, overflow, pairs)
    assert out["force_all"][2] == 1 and out["s3_exact"][2] == 0
    # forcing every row open re-scores at least one pair per row
    assert out["force_all"][0] >= n


ADVERSARIAL = ["duplicated_codes", "midpoints", "zero_rows", "rows_are_codes", "collapsed", "nearly_collapsed", "large_magnitude", "signed",
               "nan_rows", "inf_rows", "norm_overflow"]


@pytest.mark.parametrize("kind", ADVERSARIAL)
def test_s3_rows_on_adversarial_inputs_equal_the_exact_kernel(kind):
    """the kinds of tests/test_vq_filter_gpu.py (its generators live inside its test function; restated here), rows made split-3 exact.
    Collapsed codebooks put all 256 codes inside every row's band (nearly collapsed: the codes differ by 1e-6, the band is 2.4e-4 of
    |x| |e|): 255 candidates per row against a list of 4 per row, so the level MUST overflow into the gated exact launch.  Duplicated
    codes and midpoints leave two candidates per row: open rows, re-scored, no overflow needed."""
    n, c, k = 3000, 64, 256
    rows = synth.relu_features(300, (n, c))
    W = synth.relu_features(301, (k, c), sparsity=0.3, scale=1.5)
    if kind == "duplicated_codes":
        W[k // 2:] = W[:k // 2]
    elif kind == "midpoints":
        a, b = torch.arange(n) % k, (torch.arange(n) * 7 + 3) % k
        rows = 0.5 * (W[a] + W[b])
    elif kind == "zero_rows":
        rows[::3] = 0.0
    elif kind == "rows_are_codes":
        rows = W[torch.arange(n) % k].clone()
    elif kind == "collapsed":
        W[:] = W[0]
    elif kind == "nearly_collapsed":
        W = W[0][None, :] + 1e-6 * synth.uniform(302, (k, c), -1, 1)
    elif kind == "large_magnitude":
        rows, W = rows * 3.0e4, W * 2.0e4
    elif kind == "signed":
        rows, W = synth.uniform(303, (n, c), -2, 2), synth.uniform(304, (k, c), -2, 2)
    elif kind in ("nan_rows", "inf_rows", "norm_overflow"):
        rows, W, _ = vq_poison.poison_rows(rows, W, {"nan_rows": "nan_one", "inf_rows": "pos_inf"}.get(kind, kind))
    out = run_all_modes(rows, W, kind)
    if kind in ("collapsed", "nearly_collapsed", "nan_rows", "inf_rows", "norm_overflow"):
        assert out["filter"][1] == 1, f"{kind}: the level did not go to the gated exact launch"


def test_rows_whose_lo_half_decides():
    """Midpoints of two codes moved towards the first by 2^-14 of their difference: hi = bf16(x) is off by up to 2^-9 of each
    component, so on a good share of the rows hi ALONE lies on the other code's side -- a filter that dropped x_lo would rank the two
    the wrong way round, and a band that forgot a term would decide it.  The size of the move: it shifts d_a^2 - d_b^2 by
    2^-13 |a - b|^2 = 2^-13 * 64 v (v: mean squared channel difference, about 1), the rounding of hi by a sum of 64 terms
    2 delta_i (a_i - b_i), |delta_i| <= 2^-9 |x_i|, standard deviation about 2^-8 * 0.58 * 8 sqrt(v): the move is 0.4 of that, so
    about a third of the rows flip (a move of 2^-11 is 3.5 standard deviations: 12 rows of 3000 flipped); the merged value's own error,
    2^-16 per component, is 2^-7 of the rounding of hi and leaves every row on the first code's side."""
    n, c, k = 3000, 64, 256
    W = synth.relu_features(301, (k, c), sparsity=0.3, scale=1.5)
    a, b = torch.arange(n) % k, (torch.arange(n) * 7 + 3) % k
    rows = 0.5 * (W[a] + W[b]) + 2.0 ** -14 * (W[a] - W[b])
    s3 = s3_split(rows.to(dev())).cpu()
    hi, x = s3[:, :c].double(), s3_merge(s3.to(dev())).cpu().double()
    Wa, Wb = W[a].double(), W[b].double()
    side = lambda v: ((v - Wa) ** 2).sum(1) - ((v - Wb) ** 2).sum(1)      # < 0: nearer to a
    flipped = int(((side(hi) > 0) & (side(x) < 0)).sum())
    assert flipped > n // 8, f"only {flipped} of {n} rows have hi on the wrong side: the case does not test x_lo"
    run_all_modes(rows, W, "x_lo decides")


def test_codebooks_whose_lo_half_decides():
    """Twin codes e and e (1 + 2^-11 u), u = +-1 per channel: most channels of a twin pair share the bf16 hi half, the pair differs
    through e_lo.  Rows are the twins themselves: the winner is separated from its twin by |e| 2^-11 only."""
    n, c, k = 3000, 64, 256
    W = synth.relu_features(301, (k, c), sparsity=0.3, scale=1.5)
    u = torch.where(synth.uniform(305, (k // 2, c)) < 0.5, -1.0, 1.0)
    W[k // 2:] = W[:k // 2] * (1.0 + 2.0 ** -11 * u)
    same_hi = (W[k // 2:].bfloat16() == W[:k // 2].bfloat16()).float().mean().item()
    assert same_hi > 0.5, f"only {same_hi:.2f} of the twin channels share their hi half: the case does not test e_lo"
    rows = W[(torch.arange(n) * 5 + 1) % k].clone()
    run_all_modes(rows, W, "e_lo decides")


@pytest.mark.parametrize("c", [8, 40, 512])
def test_s3_gather_writes_the_split_of_the_fp32_gather(c):
    """N in {1, 17, 1000}: one row, a ragged row group, many workgroups; C = 8 one lane, 40 a partial wave, 512 a full one (and the
    filter's shape with K = 256)"""
    from vq_seg_amd import _hip
    k = 256
    W = synth.relu_features(411, (k, c), sparsity=0.3, scale=1.5).to(dev())
    prep = _hip.vq_prepare(W)
    for n in (1, 17, 1000):
        s3 = s3_split(synth.relu_features(410 + n, (n, c)).to(dev()))
        quant_f, idx_f, _l, dead_f = _hip.vq_forward(s3_merge(s3), W, False, 1.0, prepared=prep)
        (quant, idx, loss, dead), = _hip.vq_forward_group([s3], [W], [prep], False, [1.0], s3=True)
        torch.cuda.synchronize()
        assert torch.equal(idx, idx_f)
        assert quant.shape == (n, 2 * c) and quant.dtype == torch.bfloat16
        assert np.array_equal(vq_poison.bits(quant), vq_poison.bits(s3_split(quant_f))), (n, c)
        assert float(loss) == 0.0 and float(dead) == float(dead_f)


def test_row_type_2_refuses_training_and_odd_channel_counts_and_launches_nothing():
    from vq_seg_amd import _hip
    L = _hip.lib()
    n, k = 64, 256
    arr = lambda ps: (ctypes.c_void_p * 1)(*ps)

    def group_call(c, training):
        W = synth.relu_features(421, (k, c)).to(dev())
        x = torch.zeros((n, 2 * c), dtype=torch.bfloat16, device=dev())
        quant = torch.full((n, 2 * c), 7.0, dtype=torch.bfloat16, device=dev())
        idx = torch.full((n,), -5, dtype=torch.int64, device=dev())
        scal = torch.full((2,), -3.0, device=dev())
        nbytes = L.vqseg_vq_workspace_bytes(n, c, k)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev())
        ns, cs, ks = np.array([n], dtype=np.int64), np.array([c], dtype=np.int32), np.array([k], dtype=np.int32)
        cw, wsb = np.array([1.0], dtype=np.float32), (ctypes.c_size_t * 1)(nbytes)
        before = _hip.set_option("vq_filter_launches", 0)
        rc = L.vqseg_vq_forward_group(1, 2, arr([x.data_ptr()]), arr([W.data_ptr()]), None, ns.ctypes.data, cs.ctypes.data, ks.ctypes.data,
                                      training, cw.ctypes.data, arr([quant.data_ptr()]), arr([idx.data_ptr()]), arr([scal.data_ptr()]),
                                      arr([scal.data_ptr() + 4]), arr([ws.data_ptr()]), ctypes.cast(wsb, ctypes.c_void_p),
                                      torch.cuda.current_stream().cuda_stream)
        msg = L.vqseg_last_error().decode()
        torch.cuda.synchronize()
        took = _hip.set_option("vq_filter_launches", before)
        untouched = bool((quant == 7.0).all()) and bool((idx == -5).all()) and bool((scal == -3.0).all()) and not bool(ws.any())
        return rc, msg, took, untouched

    rc, msg, took, untouched = group_call(32, 1)
    assert rc == -1 and "training" in msg and took == 0 and untouched, (rc, msg, took, untouched)
    rc, msg, took, untouched = group_call(12, 0)
    assert rc == -1 and "channels % 8" in msg and took == 0 and untouched, (rc, msg, took, untouched)
    rc, msg, took, untouched = group_call(32, 0)                  # the same call, legal: it runs
    assert rc == 0 and took == 1 and not untouched, (rc, msg, took, untouched)
    with pytest.raises(_hip.HipLibraryError, match="channels % 8"):
        _hip.vq_assign(torch.zeros((n, 24), dtype=torch.bfloat16, device=dev()), synth.relu_features(422, (k, 12)).to(dev()), s3=True)
    with pytest.raises(_hip.HipLibraryError, match="eval-mode"):
        _hip.vq_forward_group([torch.zeros((n, 64), dtype=torch.bfloat16, device=dev())], [synth.relu_features(423, (k, 32)).to(dev())], [None], True,
                              [1.0], s3=True)
