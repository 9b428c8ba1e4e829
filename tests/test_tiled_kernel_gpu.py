"""The tiled-prediction kernels (vqseg_extract_windows_f, vqseg_merge_argmax_f through nnf.extract_windows / nnf.merge_argmax) on the
GPU.  The extract launch is pinned bit for bit to the package's own resize kernel applied to each crop; the merge launch is pinned
bit for bit to nnf.resize_argmax in the two configurations where its definition reduces to it (one window per image, disjoint
windows, both "uniform"), and compared everywhere else with an independent float64 restatement (tests/tiled_cases.py)."""
import ctypes

import pytest
import torch

from tests import predict_cases as P
from tests import tiled_cases as TC
from tests.test_predict_kernel_gpu import grid_cap as _predict_grid_cap

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ALL = TC.CASES + [TC.GRID_STRIDE]
ALL_IDS = TC.IDS + ["grid-stride"]


class grid_cap(_predict_grid_cap):
    """nn_grid_cap = 256 for the grid-stride case, restored whatever happens"""

    def __init__(self, on):
        self.on = bool(on)


def grid_for(case, net=None):
    from vq_seg_amd import nnf
    return nnf._window_grid(case.b, case.size[0], case.size[1], case.window, case.stride, net or (case.lh, case.lw), "test")


def bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------
# extract
# ---------------------------------------------------------------------------------------------------------------------------
def extract_and_compare(case, img, net, flips):
    """one extract launch of `flips`, held bit for bit to the resize kernel on each crop, flipped with torch -> the windows"""
    from vq_seg_amd import nnf
    ys, xs = TC.grid_of(case)
    wh, ww = case.window
    calls = nnf.EXTRACT_WINDOWS_CALLS
    out, grid = nnf.extract_windows(img, case.window, case.stride, net, flips=flips)
    assert nnf.EXTRACT_WINDOWS_CALLS == calls + 1
    assert out.shape == (len(flips), TC.rows_of(case), 3) + (net or case.window) and out.is_contiguous()
    assert (grid.ny, grid.nx) == (len(ys), len(xs))
    crops = torch.stack([img[b, :, y0:y0 + wh, x0:x0 + ww] for b in range(case.b) for y0 in ys for x0 in xs]).contiguous()
    want = crops if net is None else nnf.upsample_bilinear(crops, size=net, align_corners=False)
    for k, f in enumerate(flips):
        w = want.flip(P.FLIP_DIMS[f]) if f else want
        assert torch.equal(bits(out[k]), bits(w.contiguous())), (case, net, f, int((out[k] != w).sum()))
    return out


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.IDS)
def test_extract_is_the_resize_kernel_on_each_crop_flipped(case, layout):
    """same-size windows (an exact copy) and windows resized to the case's logit size (up- or down-scaling), all four flips in
    one launch"""
    from vq_seg_amd import nnf
    img = P.lay(TC.images(case).to(DEV), layout)
    for net in (None, (case.lh, case.lw)):
        out = extract_and_compare(case, img, net, (0, 1, 2, 3))
    one, _ = nnf.extract_windows(img, case.window, case.stride, (case.lh, case.lw), flips=(3,))      # one code that is not 0
    assert one.shape[0] == 1 and torch.equal(bits(one[0]), bits(out[3]))


@pytest.mark.parametrize("layout", P.LAYOUTS)
def test_extract_under_a_capped_grid_takes_the_grid_stride_loop(layout):
    """nn_grid_cap = 256 against 75 windows copied at 100 x 100 (2930 workgroups of 256 pixels: every thread walks more than eleven)
    and resized to 50 x 50 (733 workgroups): the results are still each crop's"""
    case = TC.GRID_STRIDE
    img = P.lay(TC.images(case).to(DEV), layout)
    blocks = -(-TC.rows_of(case) * case.window[0] * case.window[1] // 256)
    small = -(-TC.rows_of(case) * case.lh * case.lw // 256)
    assert TC.rows_of(case) == 75 and (blocks, small) == (2930, 733) and min(blocks, small) > 256
    with grid_cap(True):
        extract_and_compare(case, img, None, (0, 3))
        extract_and_compare(case, img, (case.lh, case.lw), (1, 2))


# ---------------------------------------------------------------------------------------------------------------------------
# merge: the configurations that reduce to resize_argmax, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------
def same(got, want, what):
    for g, w, name in zip(got, want, ("labels", "top", "counts")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert torch.equal(g if name != "top" else bits(g), w if name != "top" else bits(w)), (what, name, int((g != w).sum()))


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("n_views", [1, 2, 4])
@pytest.mark.parametrize("shape,size", P.SHAPES, ids=P.IDS)
def test_one_window_per_image_is_resize_argmax_bit_for_bit(shape, size, n_views, layout):
    from vq_seg_amd import nnf
    b, c, h, w = shape
    grid = nnf._window_grid(b, size[0], size[1], size, size, (h, w), "test")
    assert (grid.ny, grid.nx) == (1, 1)
    target = P.targets(shape, size).to(DEV)
    flips = {1: [3], 2: [1, 2], 4: [3, 0, 1, 2]}[n_views]
    for kind in ("normal", "ties", "special"):
        views = [P.lay(P.logits(shape, s, kind).to(DEV), layout) for s in range(n_views)]
        want = nnf.resize_argmax(views, size, flips=flips, want_top=True, target=target)
        got = nnf.merge_argmax(views, grid, flips=flips, blend="uniform", want_top=True, target=target)
        if kind == "special":                                # a NaN's payload is no result: where top is a NaN, both are
            nan = torch.isnan(want[1])
            assert torch.equal(torch.isnan(got[1]), nan) and bool(nan.any())
            got, want = (got[0], got[1].masked_fill(nan, 0.0), got[2]), (want[0], want[1].masked_fill(nan, 0.0), want[2])
        same(got, want, (shape, size, n_views, layout, kind))


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("lsize", [(8, 8), (5, 11)], ids=["same-size", "resized"])
def test_disjoint_uniform_windows_are_resize_argmax_per_window_pasted(lsize, layout):
    from vq_seg_amd import nnf
    case = TC.CASES[1]._replace(lh=lsize[0], lw=lsize[1])
    grid = grid_for(case)
    target = TC.targets(case).to(DEV)
    wh, ww = case.window
    for flips in ([0], [2, 1], [0, 1, 2, 3]):
        views = [P.lay(TC.logits(case, s).to(DEV), layout) for s in range(len(flips))]
        label, top, _ = nnf.resize_argmax(views, case.window, flips=flips, want_top=True)

        def paste(t):
            return t.reshape(case.b, grid.ny, grid.nx, wh, ww).permute(0, 1, 3, 2, 4).reshape(case.b, *case.size).contiguous()

        label, top = paste(label), paste(top)
        got = nnf.merge_argmax(views, grid, flips=flips, blend="uniform", want_top=True, target=target)
        same(got, (label, top, P.confusion(label, target.cpu(), case.c).to(DEV)), (lsize, layout, flips))


@pytest.mark.parametrize("blend", TC.BLENDS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.IDS)
def test_ties_keep_the_first_maximum_and_special_values_give_valid_labels(case, blend):
    from vq_seg_amd import nnf
    grid = grid_for(case)
    z = TC.tied(case).to(DEV)                                # classes 0 and 1 tie at every pixel of image 0
    for views, flips in (([z], [0]), ([z, z.flip(3)], [0, 1])):
        label = nnf.merge_argmax(views, grid, flips=flips, blend=blend)[0]
        assert not bool((label[0] == 1).any()) and bool((label[0] == 0).any()), (case, blend)
        assert int(label.max()) < case.c
    s = TC.logits(case, 1, "special").to(DEV)
    assert not bool(torch.isfinite(s).all())
    label, top, counts = nnf.merge_argmax([s, TC.logits(case, 2).to(DEV)], grid, flips=[2, 0], blend=blend, want_top=True,
                                          target=TC.targets(case).to(DEV))
    torch.cuda.synchronize()
    assert int(label.max()) < case.c
    assert torch.equal(counts.cpu(), P.confusion(label, TC.targets(case), case.c))


# ---------------------------------------------------------------------------------------------------------------------------
# merge: every case x V x blend against the float64 restatement
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", TC.BLENDS)
@pytest.mark.parametrize("n_views", [1, 2, 4])
@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_against_the_float64_restatement(case, n_views, blend):
    """Labels equal the float64 restatement's wherever its top-two gap exceeds P.GAP (at most 2 % of the pixels fall under it:
    tests/test_tiled_cpu.py checks that without a GPU).  top within P.top_tolerance(z64, E), E = 2 max(P.LOGIT_ERR, own): `own` is
    what the fp32 torch restatement deviates from float64 on this case (measured on the restatement, never on the kernel's output);
    the factor 2 because the kernel's fma order and the restatement's differ and each is that far from float64.  Counts are those
    of the labels the kernel wrote."""
    from vq_seg_amd import nnf
    flips = TC.VIEW_FLIPS[n_views]
    z64, label64, top64, decided, own = TC.reference(case, n_views, blend)
    assert 1.0 - decided.double().mean().item() <= 0.02
    target = TC.targets(case)
    views = [TC.logits(case, s).to(DEV) for s in range(n_views)]
    calls = nnf.MERGE_ARGMAX_CALLS
    with grid_cap(case is TC.GRID_STRIDE):
        label, top, counts = nnf.merge_argmax(views, grid_for(case), flips=flips, blend=blend, want_top=True, target=target.to(DEV))
    assert nnf.MERGE_ARGMAX_CALLS == calls + 1
    label, top, counts = label.cpu(), top.cpu().double(), counts.cpu()
    assert label.dtype == torch.uint8 and label.shape == (case.b,) + case.size
    wrong = (label.long() != label64) & decided
    E = 2.0 * max(P.LOGIT_ERR, own)
    err, tol = (top - top64).abs(), P.top_tolerance(z64, E)
    print(f"{case} V={n_views} {blend}: {int((~decided).sum())} of {decided.numel()} pixels under the gap, {int(wrong.sum())} decided labels differ; "
          f"top: max err {err.max().item():.3e}, worst err / tol {(err / tol).max().item():.3f} (own {own:.2e}, E {E:.2e})")
    assert not bool(wrong.any())
    assert bool((err <= tol).all())
    assert torch.equal(counts, P.confusion(label, target, case.c))


# ---------------------------------------------------------------------------------------------------------------------------
# merge: outputs, addresses, layouts, errors
# ---------------------------------------------------------------------------------------------------------------------------
def c_merge(case, z, blend, label, top, target, counts, n_views=1, views=None, flips=None, strides=None, **over):
    from vq_seg_amd import _hip
    k = dict(b=case.b, c=case.c, lh=case.lh, lw=case.lw, ho=case.size[0], wo=case.size[1], window=case.window, stride=case.stride)
    k.update(over)
    views = views if views is not None else (ctypes.c_void_p * 4)(*([z.data_ptr()] * 4))
    flips = flips if flips is not None else (ctypes.c_int * 4)()
    strides = strides or (case.c * case.lh * case.lw, case.lh * case.lw, 1)
    return _hip.lib().vqseg_merge_argmax_f(views, flips, n_views, *strides, k["b"], k["c"], k["lh"], k["lw"], k["ho"], k["wo"], *k["window"],
                                           *k["stride"], blend, label, top, target, counts, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.int32])
def test_each_output_alone_and_targets_outside_the_classes(dtype):
    from vq_seg_amd import nnf
    for case in (TC.CASES[0], TC.CASES[4]):
        z = TC.logits(case).to(DEV)
        target = TC.targets(case, dtype=dtype)
        assert bool((target == 255).any()) and bool((target == 7).any())
        label, top, counts = nnf.merge_argmax(z, grid_for(case), want_top=True, target=target.to(DEV))
        valid = ((target.long() >= 0) & (target.long() < case.c)).flatten(1).sum(dim=1)
        assert torch.equal(counts.sum(dim=(1, 2)).cpu(), valid) and int(valid.sum()) < target.numel()
        assert torch.equal(counts.cpu(), P.confusion(label, target, case.c))
        t64 = target.to(DEV).long().contiguous()
        only_counts = torch.full((case.b, case.c, case.c), -1, dtype=torch.int64, device=DEV)
        assert c_merge(case, z, 1, None, None, t64.data_ptr(), only_counts.data_ptr()) == 0
        assert torch.equal(only_counts, counts)
        only_label = torch.full((case.b,) + case.size, 9, dtype=torch.uint8, device=DEV)
        assert c_merge(case, z, 1, only_label.data_ptr(), None, None, None) == 0
        assert torch.equal(only_label, label)
        only_top = torch.zeros((case.b,) + case.size, dtype=torch.float32, device=DEV)
        assert c_merge(case, z, 1, None, only_top.data_ptr(), None, None) == 0
        assert torch.equal(bits(only_top), bits(top))
        l2, t2, c2 = nnf.merge_argmax(z, grid_for(case))
        assert torch.equal(l2, label) and t2 is None and c2 is None


def test_outputs_at_unaligned_addresses_take_the_pixel_by_pixel_path():
    from vq_seg_amd import nnf
    case = TC.CASES[4]                                       # 9 x 257 pixels per image: whole 256-pixel runs and partial ones
    n = case.b * case.size[0] * case.size[1]
    z = TC.logits(case).to(DEV)
    target = TC.targets(case).to(DEV)
    label, top, counts = nnf.merge_argmax(z, grid_for(case), want_top=True, target=target)
    lbuf, tbuf = torch.full((n + 3,), 9, dtype=torch.uint8, device=DEV), torch.full((n + 1,), -1.0, device=DEV)
    gbuf = torch.cat([target.reshape(-1)[:1], target.reshape(-1)])
    cnt = torch.empty_like(counts)
    assert c_merge(case, z, 1, lbuf.data_ptr() + 1, tbuf.data_ptr() + 4, gbuf.data_ptr() + 8, cnt.data_ptr()) == 0
    assert torch.equal(lbuf[1:n + 1], label.reshape(-1)) and lbuf[0].item() == 9 and bool((lbuf[n + 1:] == 9).all())
    assert torch.equal(bits(tbuf[1:]), bits(top.reshape(-1))) and tbuf[0].item() == -1.0
    assert torch.equal(cnt, counts)


@pytest.mark.parametrize("case", TC.CASES[:4], ids=TC.IDS[:4])
def test_layouts_and_mixed_layouts_between_views(case):
    from vq_seg_amd import nnf
    grid, target = grid_for(case), TC.targets(case).to(DEV)
    views = [TC.logits(case, s).to(DEV) for s in range(2)]
    want = nnf.merge_argmax(views, grid, flips=[0, 3], want_top=True, target=target)
    both = nnf.merge_argmax([P.lay(v, "channels_last") for v in views], grid, flips=[0, 3], want_top=True, target=target)
    same(both, want, (case, "channels_last"))
    for first in P.LAYOUTS:                                  # a view in another layout is brought to view 0's
        second = "nchw" if first == "channels_last" else "channels_last"
        mixed = nnf.merge_argmax([P.lay(views[0], first), P.lay(views[1], second)], grid, flips=[0, 3], want_top=True, target=target)
        same(mixed, want, (case, first, second))
    assert torch.equal(nnf.merge_argmax(views[0], grid)[0], nnf.merge_argmax([views[0], views[0]], grid, flips=[0, 0])[0])


def test_bad_arguments_raise_name_the_cause_and_leave_the_outputs_alone():
    from vq_seg_amd import _hip, nnf
    E = _hip.HipLibraryError
    case = TC.CASES[0]
    grid = grid_for(case)
    z = torch.zeros(TC.shape_of(case), device=DEV)
    t = torch.zeros((case.b,) + case.size, dtype=torch.int64, device=DEV)
    img = torch.zeros((case.b, 3) + case.size, device=DEV)
    calls = (nnf.MERGE_ARGMAX_CALLS, nnf.EXTRACT_WINDOWS_CALLS)
    for call, msg in (
            (lambda: nnf.merge_argmax([z, z, z], grid), "1, 2 or 4 views"),
            (lambda: nnf.merge_argmax(z, grid, flips=[4]), "flip code"),
            (lambda: nnf.merge_argmax([z, z], grid, flips=[1]), "one flip code per view"),
            (lambda: nnf.merge_argmax(z, grid, blend="gauss"), "blend is one of"),
            (lambda: nnf.merge_argmax(z, None), "WindowGrid"),
            (lambda: nnf.merge_argmax(z[:-1], grid), "the views have 23 rows"),
            (lambda: nnf.merge_argmax(torch.zeros(24, 5, 8, 8, device=DEV), grid), "2..4 classes"),
            (lambda: nnf.merge_argmax([z, z[:, :, :, :7]], grid), "view 0's shape"),
            (lambda: nnf.merge_argmax(z.bfloat16(), grid), "expected a float32 tensor, got torch.bfloat16"),
            (lambda: nnf.merge_argmax(z, grid, target=t[:, :, :18]), "target must have the output's shape"),
            (lambda: nnf.merge_argmax(z, grid, target=t.float()), "integer tensor"),
            (lambda: nnf.merge_argmax(z, grid, target=t.cpu()), "target: the HIP path needs .* no CPU fallback"),
            (lambda: nnf.merge_argmax(z, grid._replace(stride=(9, 4))), "leaves pixels uncovered"),
            (lambda: nnf.extract_windows(img, (14, 8)), "larger than the image"),
            (lambda: nnf.extract_windows(img, 8, 9), "leaves pixels uncovered"),
            (lambda: nnf.extract_windows(img, 8, flips=(0, 4)), "flip code"),
            (lambda: nnf.extract_windows(img, 8, flips=()), "1..4 flip codes"),
            (lambda: nnf.extract_windows(img.double(), 8), "images: expected a float32 tensor"),
            (lambda: nnf.extract_windows(img[:, :2], 8), r"\(B, 3, H, W\)")):
        with pytest.raises(E, match=msg):
            call()
    assert (nnf.MERGE_ARGMAX_CALLS, nnf.EXTRACT_WINDOWS_CALLS) == calls
    # the C level: refused with -1 before anything touches the device
    L = _hip.lib()
    label = torch.full((case.b,) + case.size, 9, dtype=torch.uint8, device=DEV)
    counts = torch.full((case.b, case.c, case.c), -1, dtype=torch.int64, device=DEV)
    lp = label.data_ptr()
    for kw, msg in ((dict(n_views=3), b"1, 2 or 4 views"), (dict(n_views=2, flips=(ctypes.c_int * 4)(0, 4)), b"flip code"),
                    (dict(c=5), b"2..4 classes"), (dict(window=(14, 8)), b"larger than the image"), (dict(stride=(4, 9)), b"stride larger than the window"),
                    (dict(stride=(0, 4)), b"must be positive"), (dict(blend=2), b"blend"), (dict(lab=None), b"nothing to compute"),
                    (dict(tgt=t.data_ptr()), b"target and counts go together"), (dict(cnt=counts.data_ptr()), b"target and counts go together"),
                    (dict(strides=(192, 64, 2)), b"layout must be planar"), (dict(strides=(191, 64, 1)), b"window stride")):
        kw = dict(kw)
        blend, lab, tgt, cnt = kw.pop("blend", 1), kw.pop("lab", lp), kw.pop("tgt", None), kw.pop("cnt", None)
        assert c_merge(case, z, blend, lab, None, tgt, cnt, **kw) == -1, (kw, msg)
        assert msg in L.vqseg_last_error() and L.vqseg_last_error().startswith(b"merge_argmax:"), (msg, L.vqseg_last_error())
    out = torch.full((1, 24, 3, 8, 8), 7.0, device=DEV)
    flips = (ctypes.c_int * 4)()
    h, w = case.size

    def c_extract(strides=(3 * h * w, h * w, 1), window=(8, 8), stride=(4, 4), net=(8, 8), f=flips, nf=1):
        return L.vqseg_extract_windows_f(img.data_ptr(), *strides, case.b, h, w, *window, *stride, *net, f, nf, out.data_ptr(), None)

    for kw, msg in ((dict(nf=5), b"1..4 flip codes"), (dict(f=(ctypes.c_int * 4)(4)), b"flip code"), (dict(window=(8, 20)), b"larger than the image"),
                    (dict(stride=(9, 4)), b"stride larger than the window"), (dict(net=(8, 0)), b"must be positive"),
                    (dict(strides=(3 * h * w, h * w, 2)), b"planar"), (dict(strides=(3 * h * w - 1, h * w, 1)), b"batch stride")):
        assert c_extract(**kw) == -1, kw
        assert msg in L.vqseg_last_error() and L.vqseg_last_error().startswith(b"extract_windows:"), (kw, L.vqseg_last_error())
    torch.cuda.synchronize()
    assert bool((label == 9).all()) and bool((counts == -1).all()) and bool((out == 7.0).all())
