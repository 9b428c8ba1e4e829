"""The fused resize + arg-max kernel (vqseg_resize_argmax_f through nnf.resize_argmax) on the GPU.  Its specification is the
two-kernel path it replaces: with one view and no flip, label / top / counts equal softmax_stats and confusion_matrix_device applied to
nnf.upsample_bilinear(logits, size) bit for bit; with 2 or 4 views, the same two kernels applied to the mean of the resized (un-flipped)
views built with torch ops.  An independent float64 reference (tests/predict_cases.py) guards against both paths sharing a mistake."""
import ctypes

import pytest
import torch

from tests import predict_cases as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ALL = P.SHAPES + [P.GRID_STRIDE]
ALL_IDS = P.IDS + ["grid-stride"]


class grid_cap:
    """nn_grid_cap = 256 for the grid-stride case (264 tiles), restored whatever happens"""

    def __init__(self, case):
        self.on = case == P.GRID_STRIDE

    def __enter__(self):
        from vq_seg_amd import _hip
        self.before = _hip.lib().vqseg_set_option(b"nn_grid_cap", 256) if self.on else None
        assert not self.on or self.before >= 256

    def __exit__(self, *exc):
        from vq_seg_amd import _hip
        if self.on:
            _hip.lib().vqseg_set_option(b"nn_grid_cap", self.before)


def two_kernel_path(acc, target):
    """what the package computes today from logits at the output size -> (label u8, top f32, counts i64)"""
    from vq_seg_amd import nnf
    from vq_seg_amd.measurement import confusion_matrix_device
    label, _ent, top = nnf.softmax_stats(acc, want_label=True, want_entropy=False, want_top=True)
    return label.to(torch.uint8), top, confusion_matrix_device(acc, target, acc.shape[1])


def same(got, want, what):
    label, top, counts = got
    wl, wt, wc = want
    assert label.dtype == torch.uint8 and top.dtype == torch.float32 and counts.dtype == torch.int64, what
    assert torch.equal(label, wl), (what, "labels", int((label != wl).sum()))
    assert torch.equal(top.view(torch.int32), wt.view(torch.int32)), (what, "top", int((top.view(torch.int32) != wt.view(torch.int32)).sum()))
    assert torch.equal(counts, wc), (what, "counts")


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_one_view_is_the_two_kernel_path_bit_for_bit(case, layout):
    from vq_seg_amd import nnf
    shape, size = case
    target = P.targets(shape, size).to(DEV)
    with grid_cap(case):
        for kind in ("normal", "ties", "special"):
            z = P.lay(P.logits(shape, 0, kind).to(DEV), layout)
            want = two_kernel_path(nnf.upsample_bilinear(z, size=size, align_corners=False), target)
            got = nnf.resize_argmax(z, size, want_top=True, target=target)
            same(got, want, (shape, size, layout, kind))
            if kind == "ties":                               # the input does produce ties between the leading classes, and class 0 wins them
                top2 = nnf.upsample_bilinear(z, size=size, align_corners=False).topk(2, dim=1).values
                assert bool((top2[:, 0] == top2[:, 1]).any()), (shape, size)
                assert bool((got[0][0] == 0).any()) and not bool((got[0][0] == 1).any())
            if kind == "special":
                assert not bool(torch.isfinite(nnf.upsample_bilinear(z, size=size, align_corners=False)).all())


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_views_equal_the_two_kernels_on_the_mean_of_the_resized_views(case, layout):
    from vq_seg_amd import nnf
    shape, size = case
    target = P.targets(shape, size).to(DEV)
    views = [P.lay(P.logits(shape, s).to(DEV), layout) for s in range(4)]
    with grid_cap(case):
        for flips in ([0, 1], [2, 3], [3, 0, 1, 2], [1, 1, 0, 2]):
            vs = views[:len(flips)]
            acc = None
            for v, f in zip(vs, flips):                      # built with torch ops around the resize kernel, on the device
                r = nnf.upsample_bilinear(v.flip(P.FLIP_DIMS[f]) if f else v, size=size, align_corners=False)
                acc = r if acc is None else acc + r
            acc = acc * (1.0 / len(vs))
            got = nnf.resize_argmax(vs, size, flips=flips, want_top=True, target=target)
            same(got, two_kernel_path(acc, target), (shape, size, layout, flips))
        one = nnf.resize_argmax(views[0], size)[0]
        twice = nnf.resize_argmax([views[0], views[0]], size, flips=[0, 0])[0]
        assert torch.equal(one, twice)
        mixed = nnf.resize_argmax([views[0], P.lay(views[1], "nchw" if layout == "channels_last" else "channels_last")], size, flips=[0, 3],
                                  want_top=True, target=target)          # a view in another layout is brought to view 0's
        same(mixed, nnf.resize_argmax(views[:2], size, flips=[0, 3], want_top=True, target=target), (shape, size, "mixed layouts"))


@pytest.mark.parametrize("n_views", [1, 2, 4])
@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_against_the_float64_restatement(case, n_views):
    """Independent reference: F.interpolate in float64 on the CPU.  Labels agree wherever the fp64 top-two logit gap exceeds GAP = 1e-4
    (7 x the 1.4e-5 fp32 interpolation itself deviates from fp64 on the small shapes); at most 2 % of the pixels may fall under it (seeds
    fixed: a condition the inputs meet, tests/test_predict_cpu.py checks it without a GPU).
    top within  u top (share + C) + E / 2:  the bar tests/test_loss_kernels_gpu.py sets softmax_stats' top probability on exact logits
    -- u top (share + (C - 1) + 1), share = sum_c p_c (|z_c - max| + 2), u = 2^-24 -- plus the interpolated logits' own error E through
    sum_c |d top / d z_c| = 2 top (1 - top) <= 1 / 2.  E = 1.4e-5, or the reference's own deviation where that is larger: what ATen's
    fp32 F.interpolate on the CPU differs from the fp64 one on this case's inputs (the source coordinate is an fp32 product that grows
    with the source extent: 8.6e-5 at 64 -> 300, up to 1.6e-5 on the small shapes), measured here, never on the kernel's output."""
    from vq_seg_amd import nnf
    shape, size = case
    flips = {1: [0], 2: [1, 2], 4: [0, 1, 2, 3]}[n_views]
    host = [P.logits(shape, s) for s in range(n_views)]
    target = P.targets(shape, size)
    acc64, label64, top64, counts64 = P.restatement(host, flips, size, target, dtype=torch.float64)
    top2 = acc64.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > P.GAP
    print(f"{shape}->{size} V={n_views}: {int((~decided).sum())} of {decided.numel()} pixels under the gap")
    assert 1.0 - decided.double().mean().item() <= 0.02
    with grid_cap(case):
        label, top, counts = nnf.resize_argmax([h.to(DEV) for h in host], size, flips=flips, want_top=True, target=target.to(DEV))
    label, top, counts = label.cpu(), top.cpu().double(), counts.cpu()
    assert torch.equal(label.long()[decided], label64[decided])
    own = (P.accumulate(host, flips, size).double() - acc64).abs().max().item()       # ATen's fp32 interpolation against fp64
    err, tol = (top - top64).abs(), P.top_tolerance(acc64, max(P.LOGIT_ERR, own))
    print(f"    top: max err {err.max().item():.3e}, worst err / tol {(err / tol).max().item():.3f} (logit error allowed {max(P.LOGIT_ERR, own):.2e})")
    assert bool((err <= tol).all())
    if bool(decided.all()):
        assert torch.equal(counts, counts64)
    assert torch.equal(counts, P.confusion(label, target, shape[1]))         # the counts are those of the labels the kernel wrote


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.int32])
def test_counts_skip_targets_outside_the_classes_and_outputs_are_optional(dtype):
    from vq_seg_amd import _hip, nnf
    for shape, size in P.SHAPES[:2] + P.SHAPES[5:]:
        b, c, h, w = shape
        z = P.logits(shape).to(DEV)
        target = P.targets(shape, size, dtype=dtype)
        assert bool((target == 255).any()) and bool((target == 7).any())
        label, top, counts = nnf.resize_argmax(z, size, want_top=True, target=target.to(DEV))
        valid = ((target.long() >= 0) & (target.long() < c)).flatten(1).sum(dim=1)
        assert torch.equal(counts.sum(dim=(1, 2)).cpu(), valid) and int(valid.sum()) < target.numel()
        assert torch.equal(counts.cpu(), P.confusion(label, target, c))
        # each output alone, at the C level: the other pointers NULL
        t64 = target.to(DEV).long().contiguous()
        views, flips = (ctypes.c_void_p * 4)(z.data_ptr()), (ctypes.c_int * 4)()
        only_counts = torch.full((b, c, c), -1, dtype=torch.int64, device=DEV)
        _hip.launch("vqseg_resize_argmax_f", DEV, views, flips, 1, c * h * w, h * w, 1, b, c, h, w, *size, None, None, t64.data_ptr(),
                    only_counts.data_ptr())
        assert torch.equal(only_counts, counts)
        only_label = torch.full((b,) + size, 9, dtype=torch.uint8, device=DEV)
        _hip.launch("vqseg_resize_argmax_f", DEV, views, flips, 1, c * h * w, h * w, 1, b, c, h, w, *size, only_label.data_ptr(), None, None, None)
        assert torch.equal(only_label, label)
        only_top = torch.zeros((b,) + size, dtype=torch.float32, device=DEV)
        _hip.launch("vqseg_resize_argmax_f", DEV, views, flips, 1, c * h * w, h * w, 1, b, c, h, w, *size, None, only_top.data_ptr(), None, None)
        assert torch.equal(only_top, top)
        l2, t2, c2 = nnf.resize_argmax(z, size)
        assert torch.equal(l2, label) and t2 is None and c2 is None


def test_outputs_at_unaligned_addresses_take_the_pixel_by_pixel_path():
    """label / top / target that are not 16-byte aligned (views into larger buffers): the same results through scalar accesses"""
    from vq_seg_amd import _hip, nnf
    shape, size = P.SHAPES[4]
    b, c, h, w = shape
    n = b * size[0] * size[1]
    z = P.logits(shape).to(DEV)
    target = P.targets(shape, size).to(DEV)
    label, top, counts = nnf.resize_argmax(z, size, want_top=True, target=target)
    lbuf, tbuf = torch.full((n + 3,), 9, dtype=torch.uint8, device=DEV), torch.full((n + 1,), -1.0, device=DEV)
    gbuf = torch.cat([target.reshape(-1)[:1], target.reshape(-1)])
    cnt = torch.empty_like(counts)
    views, flips = (ctypes.c_void_p * 4)(z.data_ptr()), (ctypes.c_int * 4)()
    _hip.launch("vqseg_resize_argmax_f", DEV, views, flips, 1, c * h * w, h * w, 1, b, c, h, w, *size, lbuf.data_ptr() + 1, tbuf.data_ptr() + 4,
                gbuf.data_ptr() + 8, cnt.data_ptr())
    assert torch.equal(lbuf[1:n + 1], label.reshape(-1)) and lbuf[0].item() == 9 and bool((lbuf[n + 1:] == 9).all())
    assert torch.equal(tbuf[1:], top.reshape(-1)) and tbuf[0].item() == -1.0
    assert torch.equal(cnt, counts)


def test_bad_arguments_raise_and_name_the_cause():
    from vq_seg_amd import _hip, nnf
    E = _hip.HipLibraryError
    z = torch.zeros(2, 3, 4, 6, device=DEV)
    t = torch.zeros(2, 8, 12, dtype=torch.int64, device=DEV)
    calls = nnf.RESIZE_ARGMAX_CALLS
    with pytest.raises(E, match="1, 2 or 4 views"):
        nnf.resize_argmax([z, z, z], (8, 12))
    with pytest.raises(E, match="flip code"):
        nnf.resize_argmax(z, (8, 12), flips=[4])
    with pytest.raises(E, match="one flip code per view"):
        nnf.resize_argmax([z, z], (8, 12), flips=[1])
    with pytest.raises(E, match="2..4 classes"):
        nnf.resize_argmax(torch.zeros(2, 5, 4, 6, device=DEV), (8, 12))
    with pytest.raises(E, match="view 0's shape"):
        nnf.resize_argmax([z, torch.zeros(2, 3, 4, 7, device=DEV)], (8, 12))
    with pytest.raises(E, match="expected a float32 tensor, got torch.bfloat16"):
        nnf.resize_argmax(z.bfloat16(), (8, 12))
    with pytest.raises(E, match="target must have the output's shape"):
        nnf.resize_argmax(z, (8, 12), target=t[:, :, :11])
    with pytest.raises(E, match="integer tensor"):
        nnf.resize_argmax(z, (8, 12), target=t.float())
    with pytest.raises(E, match="target: the HIP path needs .* no CPU fallback"):
        nnf.resize_argmax(z, (8, 12), target=t.cpu())        # everything right but the device of one tensor
    assert nnf.RESIZE_ARGMAX_CALLS == calls
    # the C level: refused with -1 before anything touches the device
    L = _hip.lib()
    views, flips = (ctypes.c_void_p * 4)(z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr()), (ctypes.c_int * 4)()
    label = torch.full((2, 8, 12), 9, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(2, 3, 3, dtype=torch.int64, device=DEV)

    def rc(v=1, f=flips, c=3, lab=label.data_ptr(), tgt=None, cnt=None, strides=(72, 24, 1)):
        return L.vqseg_resize_argmax_f(views, f, v, *strides, 2, c, 4, 6, 8, 12, lab, None, tgt, cnt, None)

    for kw, msg in ((dict(v=3), b"1, 2 or 4 views"), (dict(v=2, f=(ctypes.c_int * 4)(0, 4)), b"flip code"),
                    (dict(c=5), b"2..4 classes"), (dict(tgt=t.data_ptr()), b"target and counts go together"),
                    (dict(cnt=counts.data_ptr()), b"target and counts go together"), (dict(lab=None), b"nothing to compute"),
                    (dict(strides=(72, 24, 2)), b"layout must be planar"), (dict(strides=(71, 24, 1)), b"batch stride")):
        assert rc(**kw) == -1, kw
        assert msg in L.vqseg_last_error() and b"resize_argmax" in L.vqseg_last_error(), (kw, L.vqseg_last_error())
    torch.cuda.synchronize()
    assert bool((label == 9).all())
