"""The prediction path without a GPU: the torch path of nnf.resize_argmax against the restatement of tests/predict_cases.py, the
argument checks of vqseg_resize_argmax_f (pure host code) and of its wrapper, vq_seg_amd.predict.Predictor on a stub network, and
evaluate.test_loop(fused=True) against the unfused loop."""
import ctypes

import pytest
import torch

from tests import predict_cases as P
from vq_seg_amd import _hip, nnf


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("case", P.SHAPES, ids=P.IDS)
def test_torch_path_is_the_restatement(case, layout):
    shape, size = case
    target = P.targets(shape, size)
    for flips in ([0], [3], [1, 2], [0, 1, 2, 3]):
        views = [P.lay(P.logits(shape, s), layout) for s in range(len(flips))]
        _acc, label, top, counts = P.restatement(views, flips, size, target)
        got = nnf.resize_argmax(views if len(views) > 1 else views[0], size, flips=flips, want_top=True, target=target)
        assert got[0].dtype == torch.uint8 and got[0].shape == (shape[0],) + size
        assert torch.equal(got[0].long(), label) and torch.equal(got[1], top) and torch.equal(got[2], counts)
        assert got[2].dtype == torch.int64 and got[2].shape == (shape[0], shape[1], shape[1])
        valid = ((target >= 0) & (target < shape[1])).flatten(1).sum(dim=1)
        assert torch.equal(got[2].sum(dim=(1, 2)), valid)
    only = nnf.resize_argmax(P.logits(shape), size)
    assert only[1] is None and only[2] is None
    # an unflip is the same index map as the flip: flipping a view and naming its code gives the unflipped view's result
    z = P.logits(shape)
    for code, dims in P.FLIP_DIMS.items():
        if code:
            assert torch.equal(nnf.resize_argmax(z.flip(dims), size, flips=[code])[0], only[0])


def test_reference_inputs_meet_the_gap_condition():
    """the float64 reference's own share of pixels whose top-two logit gap is under GAP (the GPU test excludes them from the label
    comparison): at most 2 % on every shape and view count the GPU test uses, with its seeds"""
    for shape, size in P.SHAPES + [P.GRID_STRIDE]:
        for flips in ([0], [1, 2], [0, 1, 2, 3]):
            acc = P.accumulate([P.logits(shape, s) for s in range(len(flips))], flips, size, dtype=torch.float64)
            top2 = acc.topk(2, dim=1).values
            share = ((top2[:, 0] - top2[:, 1]) <= P.GAP).double().mean().item()
            assert share <= 0.02, (shape, size, flips, share)


def test_library_refuses_bad_arguments_before_the_device():
    L = _hip.lib()
    one = ctypes.c_void_p(64)                                 # never dereferenced: every call below fails its checks first
    views, flips = (ctypes.c_void_p * 4)(64, 64, 64, 64), (ctypes.c_int * 4)()

    def rc(v=1, vs=views, f=flips, strides=(72, 24, 1), b=2, c=3, h=4, w=6, ho=8, wo=12, label=one, top=None, target=None, counts=None):
        return L.vqseg_resize_argmax_f(vs, f, v, *strides, b, c, h, w, ho, wo, label, top, target, counts, None)

    cases = [(dict(v=3), b"1, 2 or 4 views"), (dict(v=0), b"1, 2 or 4 views"), (dict(v=5), b"1, 2 or 4 views"),
             (dict(vs=None), b"null views_host"), (dict(f=None), b"null views_host or flips_host"),
             (dict(vs=(ctypes.c_void_p * 4)(64, None), v=2), b"null view"),
             (dict(f=(ctypes.c_int * 4)(4)), b"flip code"), (dict(f=(ctypes.c_int * 4)(0, -1), v=2), b"flip code"),
             (dict(c=5), b"2..4 classes"), (dict(c=1), b"2..4 classes"),
             (dict(b=0), b"must be positive"), (dict(h=0), b"must be positive"), (dict(wo=0), b"must be positive"),
             (dict(target=one), b"target and counts go together"), (dict(counts=one), b"target and counts go together"),
             (dict(label=None), b"nothing to compute"),
             (dict(strides=(72, 24, 2)), b"planar"), (dict(strides=(72, 1, 4)), b"planar"), (dict(strides=(71, 24, 1)), b"batch stride")]
    for kw, msg in cases:
        assert rc(**kw) == -1, kw
        err = L.vqseg_last_error()
        assert msg in err and err.startswith(b"resize_argmax:"), (kw, err)


def test_wrapper_reports_type_and_size_before_the_device():
    E = _hip.HipLibraryError
    z = torch.zeros(2, 3, 4, 6)
    t = torch.zeros(2, 8, 12, dtype=torch.int64)
    with pytest.raises(E, match="1, 2 or 4 views"):
        nnf.resize_argmax([z, z, z], (8, 12))
    with pytest.raises(E, match="flip code"):
        nnf.resize_argmax(z, (8, 12), flips=[4])
    with pytest.raises(E, match="2..4 classes, got 5"):
        nnf.resize_argmax(torch.zeros(2, 5, 4, 6), (8, 12))
    with pytest.raises(E, match="view 0's shape"):
        nnf.resize_argmax([z, torch.zeros(2, 3, 4, 7)], (8, 12))
    with pytest.raises(E, match="logits: expected a float32 tensor, got torch.bfloat16"):
        nnf.resize_argmax(z.bfloat16(), (8, 12))
    with pytest.raises(E, match=r"logits \(view 1\): expected a float32 tensor, got torch.float64"):
        nnf.resize_argmax([z, z.double()], (8, 12))
    with pytest.raises(E, match="target must have the output's shape"):
        nnf.resize_argmax(z, (8, 12), target=t[:, :7])
    with pytest.raises(E, match="integer tensor"):
        nnf.resize_argmax(z, (8, 12), target=t.float())
    # the raw launch with a CPU tensor of the right type and size: the device error, and only then
    with pytest.raises(E, match="labels: the HIP path needs .* no CPU fallback"):
        _hip.launch("vqseg_resize_argmax_f", z.device, None, None, 1, 72, 24, 1, 2, 3, 4, 6, 8, 12,
                    _hip.tptr(torch.zeros(2, 8, 12, dtype=torch.uint8), "labels", dtype=torch.uint8, numel=192), None, None, None)
    with pytest.raises(E, match="labels: the sizes passed along need 192"):
        _hip.tptr(torch.zeros(2, 8, 11, dtype=torch.uint8), "labels", dtype=torch.uint8, numel=192)


# ---------------------------------------------------------------------------------------------------------------------------
# Predictor on a stub network (a plain torch 1 x 1 convolution that returns (logits, extra))
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    """the calls of nnf.resize_argmax: (views, size, flips, want_top) each, the function itself still runs"""
    calls = []
    real = nnf.resize_argmax

    def spy(logits, size, flips=None, want_top=False, target=None):
        calls.append((list(logits) if not torch.is_tensor(logits) else [logits], tuple(size), list(flips) if flips is not None else None, want_top))
        return real(logits, size, flips=flips, want_top=want_top, target=target)

    monkeypatch.setattr(nnf, "resize_argmax", spy)
    return calls


def images(n=2, h=10, w=14, seed=3):
    return torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(seed))


def test_predictor_views_order_flip_codes_and_modes(recorded):
    from vq_seg_amd.predict import Prediction, Predictor
    m1, m2 = P.Stub(seed=1), P.Stub(seed=2)
    m1.train()
    m2.eval()
    x = images()
    pred = Predictor([m1, m2], 3, tta=("none", "hflip"))(x)
    assert isinstance(pred, Prediction) and pred.confidence is None
    assert pred.label.dtype == torch.uint8 and pred.label.shape == (2, 10, 14)          # size=None: the input's own
    assert m1.training and not m2.training                                               # modes restored ...
    assert [s[0] for s in m1.seen] == [False, False] and [s[0] for s in m2.seen] == [False, False]      # ... after eval-mode forwards
    assert torch.equal(m1.seen[0][1], x) and torch.equal(m1.seen[1][1], x.flip(-1))
    (views, size, flips, want_top), = recorded                                           # ONE call for all views
    assert size == (10, 14) and flips == [0, 1, 0, 1] and want_top is False
    with torch.no_grad():
        want = [m1(x)[0], m1(x.flip(-1))[0], m2(x)[0], m2(x.flip(-1))[0]]                # model-major, then tta order
    assert len(views) == 4 and all(torch.equal(a, b) for a, b in zip(views, want))
    assert all(v.dtype == torch.float32 and not v.requires_grad for v in views)
    _acc, label, _top, _ = P.restatement(want, [0, 1, 0, 1], (10, 14))
    assert torch.equal(pred.label.long(), label)
    # every view name, its code, and a size of one's own
    recorded.clear()
    net = P.Stub(seed=4, pool=2).eval()
    pred = Predictor(net, 3, tta=("hvflip", "vflip", "hflip", "none"))(x, size=(15, 21), want_confidence=True)
    (views, size, flips, want_top), = recorded
    assert size == (15, 21) and flips == [3, 2, 1, 0] and want_top is True and views[0].shape == (2, 3, 5, 7)
    assert pred.label.shape == (2, 15, 21) and pred.confidence.shape == (2, 15, 21) and pred.confidence.dtype == torch.float32
    assert torch.equal(net.seen[0][1], x.flip(-2, -1)) and torch.equal(net.seen[1][1], x.flip(-2))
    assert not net.training                                                               # an eval-mode module stays in eval mode
    net.eval()
    with torch.no_grad():
        want = [net(x.flip(d) if d else x)[0] for d in ((-2, -1), (-2,), (-1,), ())]
    _acc, label, top, _ = P.restatement(want, [3, 2, 1, 0], (15, 21))
    assert torch.equal(pred.label.long(), label) and torch.equal(pred.confidence, top)


def test_predictor_restores_modes_when_the_forward_raises():
    from vq_seg_amd.predict import Predictor

    class Broken(torch.nn.Module):
        def forward(self, x):
            raise RuntimeError("boom")

    good, bad = P.Stub(), Broken()
    good.train()
    bad.train()
    with pytest.raises(RuntimeError, match="boom"):
        Predictor([good, bad], 3)(images())
    assert good.training and bad.training


def test_predictor_refuses_view_counts_other_than_1_2_4_and_unknown_views():
    from vq_seg_amd.predict import Predictor
    m = P.Stub()
    with pytest.raises(ValueError, match=r"1, 2 or 4 .* 1 x 3 = 3"):
        Predictor(m, 3, tta=("none", "hflip", "vflip"))
    with pytest.raises(ValueError, match="3 x 1 = 3"):
        Predictor([m, m, m], 3)
    with pytest.raises(ValueError, match="2 x 4 = 8"):
        Predictor([m, m], 3, tta=("none", "hflip", "vflip", "hvflip"))
    with pytest.raises(ValueError, match="rot90"):
        Predictor(m, 3, tta=("none", "rot90"))
    with pytest.raises(ValueError, match="num_classes"):
        Predictor(m, 5)
    with pytest.raises(ValueError, match=r"logits of shape \(2, 3, 10, 14\)"):
        Predictor(m, 4)(images())
    assert Predictor(m, 3, tta="hflip").tta == ("hflip",)


def test_predict_batches_takes_images_or_tuples():
    import vq_seg_amd
    from vq_seg_amd.predict import Predictor, predict_batches
    assert vq_seg_amd.Predictor is Predictor and vq_seg_amd.predict_batches is predict_batches
    m = P.Stub()
    xs = [images(seed=5), images(n=1, seed=6)]
    want = [Predictor(m, 3)(x).label for x in xs]
    for batches in (xs, [(x, "anything") for x in xs], [[x, None, 3] for x in xs]):
        got = list(predict_batches(m, iter(batches), 3))
        assert len(got) == 2 and all(torch.equal(g.label, w) and g.confidence is None for g, w in zip(got, want))
    got = list(Predictor(m, 3).predict_batches(xs, size=(5, 5), want_confidence=True))
    assert all(g.label.shape[-2:] == (5, 5) and g.confidence is not None for g in got)


# ---------------------------------------------------------------------------------------------------------------------------
# evaluate.test_loop(fused=True)
# ---------------------------------------------------------------------------------------------------------------------------
def loop_batches():
    out = []
    for seed in (11, 12):
        x = images(n=3, h=8, w=12, seed=seed)
        t = P.targets((3, 3, 8, 12), (12, 18), seed=seed)
        assert bool((t == 255).any())
        out.append((x, t))
    return out


def test_fused_test_loop_equals_the_unfused_loop():
    from vq_seg_amd.evaluate import test_loop
    m = P.Stub(seed=7)
    m.train()
    plain = test_loop(m, loop_batches(), 3)
    fused = test_loop(m, loop_batches(), 3, fused=True)
    assert fused == plain and m.training
    assert set(plain) == {"test_acc", "test_miou", "test_precision", "test_recall", "test_f1score", "test_ious"}
    assert 0.0 < plain["test_acc"] < 1.0
    flipped = test_loop(m, loop_batches(), 3, fused=True, tta=("none", "hflip"))
    assert set(flipped) == set(plain) and 0.0 < flipped["test_acc"] < 1.0
    with pytest.raises(ValueError, match="tta needs fused=True"):
        test_loop(m, loop_batches(), 3, tta=("none", "hflip"))
