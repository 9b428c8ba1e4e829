"""Tiled prediction through the public layers on the GPU: Predictor(window=...) on the pointwise stub against the untiled prediction,
evaluate.test_loop(fused=True, window=...) against the Predictor's own labels, one real vqreptunet1x1 through CPSTrainer.predict /
evaluate / Predictor.render, and the untouched path (`window=None`) against nnf.resize_argmax called directly."""
import numpy as np
import pytest
import torch

from tests import predict_cases as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def images(n=2, h=40, w=52, seed=3):
    return torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(seed))


def test_tiled_prediction_of_a_pointwise_network_agrees_with_the_untiled_one():
    """a 1 x 1 convolution gives every window the logits the whole image gives, so the blend averages equal numbers: the labels are
    the untiled ones wherever the float64 top-two gap exceeds P.GAP, and one launch each cuts and merges"""
    from vq_seg_amd import nnf
    from vq_seg_amd.predict import Predictor
    x = images()
    stub = P.Stub(3, seed=1)
    z64 = torch.nn.functional.conv2d(x.double(), stub.conv.weight.detach().double(), stub.conv.bias.detach().double())
    top2 = z64.topk(2, dim=1).values
    decided = (top2[:, 0] - top2[:, 1]) > P.GAP
    assert decided.double().mean().item() >= 0.98
    stub = stub.to(DEV)
    plain = Predictor(stub, 3, device=DEV)(x, want_confidence=True)
    assert torch.equal(plain.label.cpu().long()[decided], z64.argmax(dim=1)[decided])
    for blend in ("linear", "uniform"):
        for tta in (("none",), ("none", "hflip", "vflip", "hvflip")):
            stub.seen.clear()
            calls = (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS, nnf.RESIZE_ARGMAX_CALLS)
            tiled = Predictor(stub, 3, device=DEV, tta=tta, window=16, stride=(8, 12), blend=blend, window_batch=16)(x, want_confidence=True)
            assert (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS, nnf.RESIZE_ARGMAX_CALLS) == (calls[0] + 1, calls[1] + 1, calls[2])
            rows = 2 * len(nnf.window_starts(40, 16, 8)) * len(nnf.window_starts(52, 16, 12))
            assert sum(s[1].shape[0] for s in stub.seen) == len(tta) * rows and max(s[1].shape[0] for s in stub.seen) == 16
            assert tiled.label.shape == (2, 40, 52) and tiled.label.dtype == torch.uint8 and tiled.label.device.type == "cuda"
            assert torch.equal(tiled.label.cpu().long()[decided], z64.argmax(dim=1)[decided]), (blend, tta)
            top64 = torch.softmax(z64, dim=1).max(dim=1).values
            assert bool(((tiled.confidence.cpu().double() - top64).abs() <= P.top_tolerance(z64, 2 * P.LOGIT_ERR)).all()), (blend, tta)


def test_tiled_test_loop_counts_are_those_of_the_predictors_labels():
    from vq_seg_amd import nnf
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.measurement import Measurement
    from vq_seg_amd.predict import Predictor
    stub = P.Stub(3, seed=4).to(DEV)
    batches = []
    for seed in (5, 6):
        t = torch.randint(0, 3, (2, 40, 52), generator=torch.Generator().manual_seed(seed))
        t[:, ::5, ::3] = 255
        batches.append((images(seed=seed), t))
    kw = dict(window=(16, 20), stride=(8, 16), blend="linear", window_batch=9)
    calls = (nnf.MERGE_ARGMAX_CALLS, nnf.RESIZE_ARGMAX_CALLS)
    out = test_loop(stub, batches, 3, device=DEV, fused=True, tta=("none", "hflip"), **kw)
    assert (nnf.MERGE_ARGMAX_CALLS, nnf.RESIZE_ARGMAX_CALLS) == (calls[0] + 2, calls[1])          # one merge launch per batch
    meas, miou, acc, ious = Measurement(3), 0.0, 0.0, np.zeros(3)
    for x, t in batches:
        label = Predictor(stub, 3, device=DEV, tta=("none", "hflip"), **kw)(x).label
        conf = P.confusion(label, t, 3).numpy()
        m, per = meas.miou(conf)
        miou, ious = miou + float(m) / 2, ious + np.array(per) / 2
        acc += float((label.cpu().long() == t).flatten(1).double().mean(dim=1).mean()) / 2
    assert out["test_miou"] == pytest.approx(miou, abs=1e-12) and out["test_acc"] == pytest.approx(acc, abs=1e-12)
    assert out["test_ious"] == np.round(ious, 5).tolist()
    assert set(out) == set(test_loop(stub, batches, 3, device=DEV, fused=True))
    with pytest.raises(ValueError, match="images and masks of one size"):
        test_loop(stub, [(batches[0][0], batches[0][1][:, :39])], 3, device=DEV, fused=True, **kw)
    with pytest.raises(ValueError, match="window needs fused=True"):
        test_loop(stub, batches, 3, device=DEV, **kw)


def test_a_real_network_through_the_trainer_and_the_sheet():
    """vqreptunet1x1 on 64 x 64 windows of 96 x 128 images: CPSTrainer.predict, CPSTrainer.evaluate and Predictor.render"""
    from tests.test_predict_model_gpu import trainer
    from vq_seg_amd import nnf
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.trainer import SyntheticCropWeed
    tr = trainer()
    x, lab = SyntheticCropWeed(128, 2, DEV, seed=11, cell=8).labelled()
    x, lab = x[:, :, :96].contiguous(), lab[:, :96].contiguous()
    assert all(len(torch.unique(lab[i])) == 3 for i in range(2))
    modes = [m.training for m in tr.models]
    calls = (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS)
    pred = tr.predict(x, window=64, want_confidence=True)                                       # stride 32: 2 x 3 windows per image
    assert (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS) == (calls[0] + 1, calls[1] + 1)
    assert pred.label.shape == (2, 96, 128) and pred.label.dtype == torch.uint8 and int(pred.label.max()) < 3
    assert pred.confidence.shape == (2, 96, 128) and bool(((pred.confidence > 1 / 3 - 1e-6) & (pred.confidence <= 1)).all())
    # the windows the network saw are the crops, and the result is the merge of its own logits
    windows, grid = nnf.extract_windows(x, 64)
    assert (grid.ny, grid.nx) == (2, 3) and torch.equal(windows[0, 4], x[0, :, 32:96, 32:96])
    p = Predictor(tr.models[0], 3, amp_dtype=torch.bfloat16, window=64)
    tr.models[0].eval()
    with torch.no_grad():                                    # as Predictor.__call__ runs it
        logits = p._forward(tr.models[0], windows[0])
    tr.models[0].train(modes[0])
    want = nnf.merge_argmax(logits, grid, want_top=True)
    assert torch.equal(pred.label, want[0]) and torch.equal(pred.confidence, want[1])
    both = tr.predict(x, ensemble=True, tta=("none", "hflip"), window=64, stride=(32, 64), blend="uniform", window_batch=5)
    assert both.label.shape == (2, 96, 128) and both.confidence is None
    with pytest.raises(ValueError, match="larger than the images"):
        tr.predict(x, window=(128, 64))
    with pytest.raises(ValueError, match="own size"):
        tr.predict(x, size=(48, 64), window=64)
    out = tr.evaluate([(x, lab)], fused=True, window=64)
    conf = P.confusion(pred.label, lab, 3)
    assert out["test_acc"] == pytest.approx(float(torch.diagonal(conf, dim1=1, dim2=2).sum(dim=1).double().div(96 * 128).mean()), abs=1e-12)
    from vq_seg_amd.measurement import Measurement
    assert out["test_miou"] == pytest.approx(float(Measurement(3).miou(conf.numpy())[0]), abs=1e-12)
    with pytest.raises(ValueError, match="window needs fused=True"):
        tr.evaluate([(x, lab)], window=64)
    sheet = p.render(x, lab)
    assert sheet.shape == (2 * 96, 4 * 128 + 20, 3) and sheet.dtype == torch.uint8 and sheet.device.type == "cuda"
    assert p.render(x, half=True).shape == (96, (3 * 128 + 20) // 2, 3)
    assert [m.training for m in tr.models] == modes


def test_without_a_window_the_predictor_is_resize_argmax_on_its_views():
    from vq_seg_amd import nnf
    from vq_seg_amd.predict import Predictor
    x = images().to(DEV)
    m1, m2 = P.Stub(3, seed=1, pool=2).to(DEV).eval(), P.Stub(3, seed=2, pool=2).to(DEV).eval()
    calls = (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS)
    for size in (None, (61, 47)):
        got = Predictor([m1, m2], 3, tta=("none", "hvflip"))(x, size=size, want_confidence=True)
        with torch.no_grad():
            views = [m(x.flip(nnf.FLIP_DIMS[f]) if f else x)[0] for m in (m1, m2) for f in (0, 3)]
        want = nnf.resize_argmax(views, size or (40, 52), flips=[0, 3, 0, 3], want_top=True)
        assert torch.equal(got.label, want[0]) and torch.equal(got.confidence.view(torch.int32), want[1].view(torch.int32))
    assert (nnf.EXTRACT_WINDOWS_CALLS, nnf.MERGE_ARGMAX_CALLS) == calls
