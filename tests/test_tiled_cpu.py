"""Tiled prediction without a GPU: the window rule, the torch path of nnf.extract_windows / nnf.merge_argmax against the restatement
of tests/tiled_cases.py, the condition the GPU suite's float64 comparison rests on, the argument checks of the two entry points
(pure host code) and of their wrappers, and vq_seg_amd.predict.Predictor in tiled mode on a stub network."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import predict_cases as P
from tests import tiled_cases as TC
from vq_seg_amd import _hip, nnf

ALL = TC.CASES + [TC.GRID_STRIDE]
ALL_IDS = TC.IDS + ["grid-stride"]


def test_window_starts_cover_the_extent_and_refuse_bad_grids():
    for extent in (1, 7, 13, 19, 64, 257, 300):
        for window in range(1, extent + 1):
            for stride in {1, min(2, window), max(window // 2, 1), max(window - 1, 1), window}:
                s = nnf.window_starts(extent, window, stride)
                assert s == TC.starts(extent, window, stride)
                assert s[0] == 0 and s[-1] + window == extent
                assert len(s) == -((window - extent) // stride) + 1
                assert all(b > a for a, b in zip(s, s[1:])) and all(b - a <= stride for a, b in zip(s, s[1:]))    # ascending, no hole
                covered = torch.zeros(extent, dtype=torch.bool)
                for a in s:
                    covered[a:a + window] = True
                assert bool(covered.all())
                assert all(a == k * stride for k, a in enumerate(s[:-1]))                   # only the last window is clamped
    assert nnf.window_starts(13, 8, 4) == [0, 4, 5] and nnf.window_starts(16, 8, 8) == [0, 8] and nnf.window_starts(9, 9, 5) == [0]
    for bad in ((8, 9, 4), (8, 4, 5), (8, 4, 0), (0, 0, 0)):
        with pytest.raises(ValueError, match="1 <= stride <= window <= extent"):
            nnf.window_starts(*bad)


@pytest.mark.parametrize("case", TC.CASES, ids=TC.IDS)
def test_torch_path_of_extract_windows_is_crop_resize_flip(case):
    img = TC.images(case)
    ys, xs = TC.grid_of(case)
    for net in (None, (case.lh, case.lw)):
        out, grid = nnf.extract_windows(P.lay(img, "channels_last"), case.window, case.stride, net, flips=(0, 1, 2, 3))
        nh, nw = case.window if net is None else net
        assert out.shape == (4, TC.rows_of(case), 3, nh, nw) and out.dtype == torch.float32
        assert (grid.batch, grid.height, grid.width, grid.ny, grid.nx) == (case.b, *case.size, len(ys), len(xs))
        assert grid.window == case.window and grid.stride == case.stride and grid.net_size == (nh, nw)
        for b in range(case.b):
            for j, y0 in enumerate(ys):
                for i, x0 in enumerate(xs):
                    crop = img[b:b + 1, :, y0:y0 + case.window[0], x0:x0 + case.window[1]]
                    want = crop if net is None else F.interpolate(crop, size=net, mode="bilinear", align_corners=False)
                    row = (b * len(ys) + j) * len(xs) + i
                    for f in range(4):
                        assert torch.equal(out[f, row], want[0].flip([d - 1 for d in P.FLIP_DIMS[f]])), (b, j, i, f)
    half, grid = nnf.extract_windows(img, case.window)                                      # stride defaults to window // 2
    assert grid.stride == (max(case.window[0] // 2, 1), max(case.window[1] // 2, 1)) and half.shape[0] == 1


@pytest.mark.parametrize("blend", TC.BLENDS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.IDS)
def test_torch_path_of_merge_argmax_is_the_restatement(case, blend):
    target = TC.targets(case)
    _w, grid = nnf.extract_windows(TC.images(case), case.window, case.stride, (case.lh, case.lw))
    for flips in ([0], [3], [1, 2], [0, 1, 2, 3]):
        views = [TC.logits(case, s) for s in range(len(flips))]
        _z, label, top, counts = TC.restatement(views, flips, case, blend, target)
        got = nnf.merge_argmax(views if len(views) > 1 else views[0], grid, flips=flips, blend=blend, want_top=True, target=target)
        assert got[0].dtype == torch.uint8 and got[0].shape == (case.b,) + case.size
        assert torch.equal(got[0].long(), label) and torch.equal(got[1], top) and torch.equal(got[2], counts)
        assert got[2].dtype == torch.int64 and got[2].shape == (case.b, case.c, case.c)
    only = nnf.merge_argmax(TC.logits(case), grid, blend=blend)
    assert only[1] is None and only[2] is None
    for code, dims in P.FLIP_DIMS.items():                   # an unflip is the same index map as the flip
        if code:
            assert torch.equal(nnf.merge_argmax(TC.logits(case).flip(dims), grid, flips=[code], blend=blend)[0], only[0])


def test_one_window_and_disjoint_windows_reduce_to_resize_argmax_on_the_torch_path():
    z = P.logits((2, 3, 5, 7))
    _w, grid = nnf.extract_windows(torch.zeros(2, 3, 13, 9), (13, 9), (13, 9), (5, 7))
    assert (grid.ny, grid.nx) == (1, 1)
    want = nnf.resize_argmax(z, (13, 9), want_top=True)
    got = nnf.merge_argmax(z, grid, blend="uniform", want_top=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    case = TC.CASES[1]
    _w, grid = nnf.extract_windows(TC.images(case), case.window, case.stride)
    z = TC.logits(case)
    per = nnf.resize_argmax(z, case.window)[0].reshape(case.b, grid.ny, grid.nx, *case.window)
    pasted = per.permute(0, 1, 3, 2, 4).reshape(case.b, *case.size)
    assert torch.equal(nnf.merge_argmax(z, grid, blend="uniform")[0], pasted)


@pytest.mark.parametrize("case", ALL, ids=ALL_IDS)
def test_reference_inputs_meet_the_gap_condition(case):
    """the condition the GPU suite's float64 comparison rests on: at most 2 % of the pixels have a float64 top-two gap of P.GAP or
    less, for every view count and blend; and the fp32 restatement itself stays within P.LOGIT_ERR of float64 -- the GPU test allows
    the kernel twice the larger of the two, so a restatement that drifted would loosen the kernel's bound, and fails here first"""
    for n_views in (1, 2, 4):
        for blend in TC.BLENDS:
            _z, _l, _t, decided, own = TC.reference(case, n_views, blend)
            share = 1.0 - decided.double().mean().item()
            print(f"{case} V={n_views} {blend}: share under the gap {share:.5f}, fp32 restatement against fp64 {own:.2e}")
            assert share <= 0.02, (case, n_views, blend, share)
            assert own <= P.LOGIT_ERR, (case, n_views, blend, own)


def test_library_refuses_bad_arguments_before_the_device():
    L = _hip.lib()
    one = ctypes.c_void_p(64)                                 # never dereferenced: every call below fails its checks first
    views, flips = (ctypes.c_void_p * 4)(64, 64, 64, 64), (ctypes.c_int * 4)()

    def merge(v=1, vs=views, f=flips, strides=(192, 64, 1), b=2, c=3, lh=8, lw=8, ho=13, wo=19, win=(8, 8), st=(4, 4), blend=1, label=one, top=None,
              target=None, counts=None):
        return L.vqseg_merge_argmax_f(vs, f, v, *strides, b, c, lh, lw, ho, wo, *win, *st, blend, label, top, target, counts, None)

    cases = [(dict(v=3), b"1, 2 or 4 views"), (dict(v=0), b"1, 2 or 4 views"), (dict(vs=None), b"null views_host"),
             (dict(f=None), b"null views_host or flips_host"), (dict(vs=(ctypes.c_void_p * 4)(64, None), v=2), b"null view"),
             (dict(f=(ctypes.c_int * 4)(4)), b"flip code"), (dict(c=5), b"2..4 classes"), (dict(c=1), b"2..4 classes"),
             (dict(b=0), b"must be positive"), (dict(lh=0), b"must be positive"), (dict(wo=0), b"must be positive"),
             (dict(win=(14, 8)), b"larger than the image"), (dict(win=(8, 20)), b"larger than the image"),
             (dict(st=(9, 4)), b"stride larger than the window"), (dict(st=(4, 0)), b"must be positive"), (dict(win=(0, 8)), b"must be positive"),
             (dict(ho=5000, win=(4097, 8)), b"above 4096"), (dict(blend=2), b"blend"), (dict(blend=-1), b"blend"),
             (dict(target=one), b"target and counts go together"), (dict(counts=one), b"target and counts go together"),
             (dict(label=None), b"nothing to compute"), (dict(strides=(192, 64, 2)), b"planar"), (dict(strides=(192, 1, 4)), b"planar"),
             (dict(strides=(191, 64, 1)), b"window stride")]
    for kw, msg in cases:
        assert merge(**kw) == -1, kw
        err = L.vqseg_last_error()
        assert msg in err and err.startswith(b"merge_argmax:"), (kw, err)

    def extract(img=one, strides=(741, 247, 1), b=2, h=13, w=19, win=(8, 8), st=(4, 4), net=(8, 8), f=flips, nf=1, out=one):
        return L.vqseg_extract_windows_f(img, *strides, b, h, w, *win, *st, *net, f, nf, out, None)

    cases = [(dict(img=None), b"null images"), (dict(out=None), b"null images, out"), (dict(f=None), b"flips_host"),
             (dict(nf=0), b"1..4 flip codes"), (dict(nf=5), b"1..4 flip codes"), (dict(f=(ctypes.c_int * 4)(0, 4), nf=2), b"flip code"),
             (dict(b=0), b"must be positive"), (dict(net=(0, 8)), b"must be positive"), (dict(win=(14, 8)), b"larger than the image"),
             (dict(st=(4, 9)), b"stride larger than the window"), (dict(st=(0, 4)), b"must be positive"),
             (dict(strides=(741, 247, 2)), b"planar"), (dict(strides=(741, 1, 4)), b"planar"), (dict(strides=(740, 247, 1)), b"batch stride")]
    for kw, msg in cases:
        assert extract(**kw) == -1, kw
        err = L.vqseg_last_error()
        assert msg in err and err.startswith(b"extract_windows:"), (kw, err)


def test_wrappers_report_the_cause_before_the_device():
    E = _hip.HipLibraryError
    img = torch.zeros(2, 3, 13, 19)
    with pytest.raises(E, match=r"\(B, 3, H, W\)"):
        nnf.extract_windows(torch.zeros(2, 4, 13, 19), 8)
    with pytest.raises(E, match="larger than the image"):
        nnf.extract_windows(img, (14, 8))
    with pytest.raises(E, match="leaves pixels uncovered"):
        nnf.extract_windows(img, 8, 9)
    with pytest.raises(E, match="must be positive"):
        nnf.extract_windows(img, 8, 0)
    with pytest.raises(E, match="window must be an int or a"):
        nnf.extract_windows(img, "big")
    with pytest.raises(E, match="flip code"):
        nnf.extract_windows(img, 8, flips=(0, 4))
    with pytest.raises(E, match="1..4 flip codes"):
        nnf.extract_windows(img, 8, flips=())
    with pytest.raises(E, match="images: expected a float32 tensor, got torch.float64"):
        nnf.extract_windows(img.double(), 8)
    _w, grid = nnf.extract_windows(img, 8, 4)
    z = torch.zeros(24, 3, 8, 8)
    t = torch.zeros(2, 13, 19, dtype=torch.int64)
    with pytest.raises(E, match="1, 2 or 4 views"):
        nnf.merge_argmax([z, z, z], grid)
    with pytest.raises(E, match="one flip code per view"):
        nnf.merge_argmax([z, z], grid, flips=[1])
    with pytest.raises(E, match="flip code"):
        nnf.merge_argmax(z, grid, flips=[4])
    with pytest.raises(E, match="blend is one of"):
        nnf.merge_argmax(z, grid, blend="gauss")
    with pytest.raises(E, match="WindowGrid"):
        nnf.merge_argmax(z, (13, 19))
    with pytest.raises(E, match="2 x 3 x 4 = 24 windows, the views have 23 rows"):
        nnf.merge_argmax(z[:23], grid)
    with pytest.raises(E, match="2..4 classes, got 5"):
        nnf.merge_argmax(torch.zeros(24, 5, 8, 8), grid)
    with pytest.raises(E, match="view 0's shape"):
        nnf.merge_argmax([z, torch.zeros(24, 3, 8, 7)], grid)
    with pytest.raises(E, match=r"window logits \(view 1\): expected a float32 tensor, got torch.float64"):
        nnf.merge_argmax([z, z.double()], grid)
    with pytest.raises(E, match="target must have the output's shape"):
        nnf.merge_argmax(z, grid, target=t[:, :12])
    with pytest.raises(E, match="integer tensor"):
        nnf.merge_argmax(z, grid, target=t.float())
    with pytest.raises(E, match="larger than the image"):
        nnf.merge_argmax(z, grid._replace(height=7))


# ---------------------------------------------------------------------------------------------------------------------------
# Predictor in tiled mode on a stub network (a plain torch 1 x 1 convolution that returns (logits, extra))
# ---------------------------------------------------------------------------------------------------------------------------
def images(n=2, h=13, w=19, seed=3):
    return torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(seed))


def test_tiled_predictor_windows_views_chunks_and_modes():
    from vq_seg_amd.predict import Prediction, Predictor
    x = images()
    m1, m2 = P.Stub(3, seed=1), P.Stub(3, seed=2)
    m1.train(), m2.eval()
    calls = (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS)
    p = Predictor([m1, m2], 3, tta=("none", "hflip"), window=8, stride=4)
    out = p(x, want_confidence=True)
    assert isinstance(out, Prediction) and out.label.shape == (2, 13, 19) and out.label.dtype == torch.uint8
    assert out.confidence.shape == (2, 13, 19) and out.confidence.dtype == torch.float32
    assert (m1.training, m2.training) == (True, False)                                      # modes restored
    assert (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS) == calls                     # CPU tensors never reach the library
    windows, grid = nnf.extract_windows(x, 8, 4, flips=(0, 1))
    rows = 2 * 3 * 4
    for m in (m1, m2):                                       # each model sees F * B * T windows, in eval mode, view by view
        assert [s[0] for s in m.seen] == [False, False] and sum(s[1].shape[0] for s in m.seen) == 2 * rows
        assert torch.equal(m.seen[0][1], windows[0]) and torch.equal(m.seen[1][1], windows[1])
    # the result is the merge of the stubs' own logits, views model-major then tta order
    views = [m.conv(windows[k]) for m in (m1, m2) for k in (0, 1)]
    want = nnf.merge_argmax([v.detach() for v in views], grid, flips=[0, 1, 0, 1], blend="linear", want_top=True)
    assert torch.equal(out.label, want[0]) and torch.equal(out.confidence, want[1])
    # window_batch chunks the forwards and changes nothing else
    for m in (m1, m2):
        m.seen.clear()
    chunked = Predictor([m1, m2], 3, tta=("none", "hflip"), window=8, stride=4, window_batch=5)(x, want_confidence=True)
    assert torch.equal(chunked.label, out.label) and torch.equal(chunked.confidence, out.confidence)
    assert [s[1].shape[0] for s in m1.seen] == [5, 5, 5, 5, 4] * 2 and sum(s[1].shape[0] for s in m2.seen) == 2 * rows
    assert torch.equal(torch.cat([s[1] for s in m1.seen[:5]]), windows[0])
    # the blend and the stride default are passed on
    uni = Predictor(m1, 3, window=(8, 10), blend="uniform")(x)
    w2, g2 = nnf.extract_windows(x, (8, 10))
    assert g2.stride == (4, 5)
    assert torch.equal(uni.label, nnf.merge_argmax(m1.conv(w2[0]).detach(), g2, blend="uniform")[0])
    # a network that sees another size than the window: resized on the way in, the logits on the way out
    small = Predictor(m1, 3, window=8, stride=4, net_size=(6, 5))
    m1.seen.clear()
    got = small(x)
    assert m1.seen[0][1].shape == (rows, 3, 6, 5) and got.label.shape == (2, 13, 19)
    # one window per image, uniform: the untiled prediction of a pointwise network
    whole = Predictor(m1, 3, window=(13, 19), blend="uniform")(x, want_confidence=True)
    plain = Predictor(m1, 3)(x, want_confidence=True)
    assert torch.equal(whole.label, plain.label) and torch.equal(whole.confidence, plain.confidence)
    assert [pr.label.shape for pr in p.predict_batches([x, (x[:1], None)])] == [(2, 13, 19), (1, 13, 19)]


def test_tiled_predictor_refuses_bad_arguments():
    from vq_seg_amd.predict import Predictor, predict_batches
    x, m = images(), P.Stub(3)
    with pytest.raises(ValueError, match=r"window of \(16, 8\) is larger than the images of \(13, 19\)"):
        Predictor(m, 3, window=(16, 8))(x)
    with pytest.raises(ValueError, match=r"own size \(13, 19\), got size \(26, 38\)"):
        Predictor(m, 3, window=8)(x, size=(26, 38))
    assert Predictor(m, 3, window=8)(x, size=(13, 19)).label.shape == (2, 13, 19)
    with pytest.raises(ValueError, match="give a window"):
        Predictor(m, 3, stride=4)
    with pytest.raises(ValueError, match="give a window"):
        Predictor(m, 3, window_batch=4)
    with pytest.raises(ValueError, match="blend is one of"):
        Predictor(m, 3, window=8, blend="gauss")
    with pytest.raises(ValueError, match="window_batch must be positive"):
        Predictor(m, 3, window=8, window_batch=0)
    with pytest.raises(_hip.HipLibraryError, match="leaves pixels uncovered"):
        Predictor(m, 3, window=8, stride=9)(x)
    with pytest.raises(ValueError, match="no window"):
        Predictor(m, 3).tiled_views(x)
    assert m.training                                        # ... and the mode came back after every refusal
    assert next(predict_batches(m, [x], 3, window=8, stride=4, window_batch=7)).label.shape == (2, 13, 19)


def test_tiled_test_loop_counts_are_those_of_the_predictors_labels():
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.measurement import Measurement
    from vq_seg_amd.predict import Predictor
    m = P.Stub(3, seed=4)
    x = images()
    t = torch.randint(0, 3, (2, 13, 19), generator=torch.Generator().manual_seed(5))
    t[:, ::5, ::3] = 255
    out = test_loop(m, [(x, t)], 3, fused=True, window=8, stride=4, blend="uniform", window_batch=6)
    label = Predictor(m, 3, window=8, stride=4, blend="uniform")(x).label
    conf = P.confusion(label, t, 3).numpy()
    assert out["test_miou"] == pytest.approx(float(Measurement(3).miou(conf)[0]), abs=1e-12)
    assert out["test_acc"] == pytest.approx(float((label.long() == t).flatten(1).double().mean(dim=1).mean()), abs=1e-12)
    with pytest.raises(ValueError, match="window needs fused=True"):
        test_loop(m, [(x, t)], 3, window=8)
    with pytest.raises(ValueError, match="images and masks of one size"):
        test_loop(m, [(x, t[:, :12])], 3, fused=True, window=8)
    with pytest.raises(ValueError, match="visualize is not built"):
        test_loop(m, [(x, t)], 3, fused=True, window=8, visualize=lambda *a: None)
    # whatever refuses inside the loop, the model's mode comes back
    m.train()
    for kw, err, msg in ((dict(window=16), ValueError, "larger than the images"), (dict(window=8, stride=9), _hip.HipLibraryError, "uncovered")):
        with pytest.raises(err, match=msg):
            test_loop(m, [(x, t)], 3, fused=True, **kw)
        assert m.training
    with pytest.raises(ValueError, match="images and masks of one size"):
        test_loop(m, [(x, t[:, :12])], 3, fused=True, window=8)
    assert m.training
